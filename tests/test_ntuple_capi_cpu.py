"""The n-tuple network's C ABI without a GPU: oth_ntuple_weight_count,
oth_ntuple_plan_bytes and oth_ntuple_plan, which run on the host, and every argument
check of oth_ntuple_eval, oth_ntuple_update and oth_search_ntuple (with nothing
launched), in the manner of tests/test_cnet_capi_cpu.py."""
import ctypes
import threading

import numpy as np
import pytest

import ntuple_cases as nc
import ntuple_ref as nr
from test_ntuple_host import load_hostlib, ptr


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


TUPLES = nc.tuples(8, 5, "mixed")


def params(tp=TUPLES, shift=3, **fields):
    from gymothelloenv_amd import _lib as L
    p = nc.fill_params(L.OthNtupleParams(), tp, shift)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def bad_params():
    """(what, params, a word of the message)"""
    out = [("tuples = 0", params(tuples=0), b"tuples"), ("tuples = 33", params(tuples=33), b"tuples"),
           ("value_shift = -1", params(value_shift=-1), b"value_shift"),
           ("value_shift = 25", params(value_shift=25), b"value_shift")]
    for v in (0, 9, -3):
        p = params()
        p.length[4] = v
        out.append(("length = %d" % v, p, b"length"))
    for v in (-1, 64, 1 << 20):
        p = params()
        p.squares[2][1] = v
        out.append(("square = %d" % v, p, b"squares"))
    p = params()
    p.squares[0][7] = p.squares[0][2]
    out.append(("a square twice", p, b"distinct"))
    return out


def ref(p):
    return None if p is None else ctypes.byref(p)


def test_counts_and_plan_bytes(lib):
    from gymothelloenv_amd import _lib as L
    assert (L.OTH_NTUPLE_MAX_TUPLES, L.OTH_NTUPLE_MAX_LENGTH, L.OTH_NTUPLE_MAX_ROWS) == (32, 8, 1 << 24)
    assert (L.OTH_NTUPLE_MAX_RATE, L.OTH_NTUPLE_MAX_RATE_SHIFT) == (1 << 24, 40)

    def count(n, p):
        c = ctypes.c_uint64(0)
        return lib.oth_ntuple_weight_count(n, ref(p), ctypes.byref(c)), c.value

    def size(n, p):
        b = ctypes.c_uint64(0)
        return lib.oth_ntuple_plan_bytes(n, ref(p), ctypes.byref(b)), b.value

    sizes = set()
    for n, T, kind in nc.CONFIGS:
        tp = nc.tuples(n, T, kind)
        assert count(n, params(tp)) == (0, nr.weight_count(tp)), (n, T, kind)
        rc, b = size(n, params(tp))
        assert rc == 0 and 0 < b <= 4096 and b % 8 == 0
        sizes.add((T, b))
    assert len(sizes) == len({T for _, T, _ in nc.CONFIGS})  # the size depends on T alone
    assert count(8, params(nc.tuples(8, 32, "eights"))) == (0, 32 * 6561 + 1)
    p = params()  # fields beyond T and l_t are not read
    p.length[5], p.squares[1][2], p.squares[9][0] = 99, -5, 1000
    assert count(8, p) == (0, nr.weight_count(TUPLES)) and size(8, p)[0] == 0

    def run():
        res = []
        for fn in (count, size):
            res += [(what, fn(8, p), lib.oth_last_error(), word) for what, p, word in bad_params()]
            res += [("board_size = %d" % n, fn(n, params()), lib.oth_last_error(), b"board_size") for n in (3, 17)]
            res.append(("NULL params", fn(8, None), lib.oth_last_error(), b"params"))
        res.append(("NULL count", (lib.oth_ntuple_weight_count(8, ref(params()), None), 0), lib.oth_last_error(), b"count"))
        res.append(("NULL bytes", (lib.oth_ntuple_plan_bytes(8, ref(params()), None), 0), lib.oth_last_error(), b"bytes"))
        return res

    for what, (rc, v), msg, word in on_a_thread(run):
        assert rc == -1 and v == 0 and msg and word in msg, (what, msg)
    # a square of a larger board is out of range on a smaller one
    assert count(4, params(nc.tuples(4, 5, "mixed")))[0] == 0 and on_a_thread(lambda: count(4, params()))[0] == -1


def plan_of(lib, n, p):
    b = ctypes.c_uint64(0)
    assert lib.oth_ntuple_plan_bytes(n, ref(p), ctypes.byref(b)) == 0
    whole = np.full(b.value // 8 + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert lib.oth_ntuple_plan(n, ref(p), ptr(whole), b.value) == 0
    assert (whole[b.value // 8:] == 0xA5A5A5A5A5A5A5A5).all(), "the call wrote behind the plan"
    return whole[:b.value // 8].tobytes()


def test_plan_is_a_function_of_the_parameters(lib):
    base = plan_of(lib, 8, params())
    assert plan_of(lib, 8, params()) == base and len(base) % 8 == 0  # the same bytes on two calls
    seen = {base}
    variants = [(8, params(shift=4)), (9, params()), (8, params(TUPLES[:4])), (8, params(TUPLES + [[3]]))]
    p = params()
    p.squares[3][0] = (p.squares[3][0] + 1) % 64  # (a 1-tuple: still distinct)
    variants.append((8, p))
    swapped = [list(t) for t in TUPLES]
    swapped[0][0], swapped[0][1] = swapped[0][1], swapped[0][0]
    variants.append((8, params(swapped)))
    variants.append((8, params([TUPLES[1], TUPLES[0]] + TUPLES[2:])))
    for n, p in variants:
        b = plan_of(lib, n, p)
        assert b not in seen
        seen.add(b)
    # what is not read does not show
    p2 = params()
    p2.length[7], p2.squares[6][3], p2.squares[1][5] = 5, 99, 7  # (tuple 1 has two squares)
    assert len(TUPLES) == 5 and len(TUPLES[1]) == 2 and plan_of(lib, 8, p2) == base
    # the host build of csrc/ntuple.hpp makes the same bytes
    host = load_hostlib()
    for n, T, kind in nc.CONFIGS:
        tp = nc.tuples(n, T, kind)
        want = plan_of(lib, n, params(tp))
        buf = np.zeros(len(want) // 8, dtype=np.uint64)
        assert host.host_ntuple_plan(n, ctypes.byref(nc.params(tp, 3)), ptr(buf), len(want)) == len(want)
        assert buf.tobytes() == want


def test_argument_checks_without_gpu(lib):
    n = 8
    count = nr.weight_count(TUPLES)
    plan = np.zeros(512, dtype=np.uint64)
    plan_bytes = len(plan_of(lib, n, params()))
    out = (ctypes.c_int64 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    good = params()
    fake_env = (ctypes.c_int32 * 64)(37, 8, 1)  # the head of a handle: E, n, W; nothing else is read before a refusal
    env = ctypes.cast(fake_env, ctypes.c_void_p)

    def pl(n=n, p=good, plan_=ptr(plan), nbytes=plan_bytes):
        return lib.oth_ntuple_plan, (n, ref(p), plan_, nbytes)

    def ev(n=n, R=4, p=good, plan_=ptr(plan), nbytes=1 << 20, w=arr, wc=count, boards=arr, meta=arr, values=arr):
        return lib.oth_ntuple_eval, (n, R, ref(p), plan_, nbytes, w, wc, boards, meta, values, None, None)

    def up(n=n, R=4, p=good, plan_=ptr(plan), nbytes=1 << 20, w=arr, wc=count, boards=arr, meta=arr, targets=arr, rate=1,
           rate_shift=0, deltas=arr):
        return lib.oth_ntuple_update, (n, R, ref(p), plan_, nbytes, w, wc, boards, meta, targets, rate, rate_shift, deltas,
                                       None)

    def se(env_=env, depth=2, p=good, plan_=ptr(plan), nbytes=1 << 20, w=arr, wc=count, term=64, budget=1 << 20, value=arr):
        return lib.oth_search_ntuple, (env_, depth, ref(p), plan_, nbytes, w, wc, term, budget, value, None, None, None,
                                       None, None)

    cases = []
    for name, call in (("plan", pl), ("eval", ev), ("update", up), ("search", se)):
        cases += [(name + ": " + what, call(p=p), word) for what, p, word in bad_params()]
        cases += [(name + ": NULL params", call(p=None), b"params"),
                  (name + ": NULL plan", call(plan_=None), b"plan"),
                  (name + ": misaligned plan", call(plan_=ctypes.c_void_p(plan.ctypes.data + 4)), b"aligned"),
                  (name + ": short plan", call(nbytes=plan_bytes - 1), b"plan_bytes")]
        if name != "search":
            cases += [(name + ": board_size = 3", call(n=3), b"board_size"),
                      (name + ": board_size = 17", call(n=17), b"board_size")]
        if name != "plan":
            cases += [(name + ": NULL weights", call(w=None), b"weights"),
                      (name + ": short weights", call(wc=count - 1), b"weight_count")]
    for name, call in (("eval", ev), ("update", up)):
        cases += [(name + ": NULL boards", call(boards=None), b"boards"), (name + ": NULL meta", call(meta=None), b"meta"),
                  (name + ": n_rows = -1", call(R=-1), b"n_rows"),
                  (name + ": n_rows = 2^24 + 1", call(R=(1 << 24) + 1), b"n_rows")]
    cases += [("eval: NULL values", ev(values=None), b"values"),
              ("update: NULL targets", up(targets=None), b"targets"), ("update: NULL deltas", up(deltas=None), b"deltas"),
              ("update: rate = -1", up(rate=-1), b"rate"), ("update: rate = 2^24 + 1", up(rate=(1 << 24) + 1), b"rate"),
              ("update: rate_shift = -1", up(rate_shift=-1), b"rate_shift"),
              ("update: rate_shift = 41", up(rate_shift=41), b"rate_shift"),
              ("search: NULL env", se(env_=None), b"oth_env"), ("search: NULL value", se(value=None), b"value"),
              ("search: depth = 0", se(depth=0), b"depth"), ("search: depth = 15", se(depth=15), b"depth"),
              ("search: terminal = 0", se(term=0), b"terminal"), ("search: terminal = 32768", se(term=32768), b"terminal"),
              ("search: max_nodes = 0", se(budget=0), b"max_nodes"),
              ("search: max_nodes = 2^32", se(budget=1 << 32), b"max_nodes")]

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert msg and word in msg, (what, msg)
    assert list(out) == [0] * 64 and not plan.any()  # nothing was written
    # no rows: nothing to launch, and no GPU needed to say so
    for call in (ev, up):
        fn, args = call(R=0)
        assert fn(*args) == 0
    fn, args = pl()
    assert fn(*args) == 0 and plan[:plan_bytes // 8].any() and not plan[plan_bytes // 8:].any()
