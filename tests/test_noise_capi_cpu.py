"""oth_puct_noise's C ABI without a GPU: every argument check that needs no handle
(each comes before the handle is read, with nothing launched), the constants, and the
Python surface."""
import ctypes
import inspect
import threading

import pytest


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


def test_constants_and_symbol(lib):
    from gymothelloenv_amd import _lib as L
    assert (L.OTH_NOISE_TABLE, L.OTH_NOISE_G_MAX) == (4096, 1 << 24)
    assert "oth_puct_noise" in L.SIGNATURES and len(L.SIGNATURES["oth_puct_noise"][1]) == 12
    assert lib.oth_puct_noise is not None


def test_argument_checks_without_gpu(lib):
    buf = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(buf, ctypes.c_void_p)

    def call(env=None, K=1, kind=None, boards=None, pin=arr, pout=arr, eps=64, table=arr):
        return (env, K, kind, boards, pin, pout, eps, table, 1, 0, 0, None)

    cases = [("NULL priors_in", call(pin=None), b"priors"), ("NULL priors_out", call(pout=None), b"priors"),
             ("NULL table", call(table=None), b"table"), ("kind alone", call(kind=arr), b"kind and boards"),
             ("boards alone", call(boards=arr), b"kind and boards"), ("K = 0", call(K=0), b"rows_per_board"),
             ("K = 65", call(K=65), b"rows_per_board"), ("K = -1", call(K=-1), b"rows_per_board"),
             ("epsilon = -1", call(eps=-1), b"epsilon"), ("epsilon = 257", call(eps=257), b"epsilon"),
             ("NULL handle, root mode", call(), b"oth_env"),
             ("NULL handle, leaf mode", call(kind=arr, boards=arr, K=64, eps=256), b"oth_env"),
             ("NULL handle, epsilon = 0", call(eps=0), b"oth_env")]

    def run():
        return [(what, lib.oth_puct_noise(*args), lib.oth_last_error(), word) for what, args, word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert msg and word in msg, (what, msg)
    assert list(buf) == [0] * 64  # nothing was written


def test_python_surface():
    import gymothelloenv_amd as g
    from gymothelloenv_amd import noise, vec_env

    assert g.RootNoise is noise.RootNoise and g.dirichlet_table is noise.dirichlet_table
    names = list(inspect.signature(vec_env.VecOthelloEnv.puct_noise).parameters)[1:]
    assert names == ["priors", "epsilon", "table", "leaves", "rows_per_board", "out", "seed", "id_key", "counter"]
    assert isinstance(vec_env.VecOthelloEnv.puct_noise_counter, property)
    assert list(inspect.signature(noise.RootNoise.__init__).parameters)[1:] == ["epsilon", "alpha"]
    # the keyword is popped from the keyword dict: the signatures an existing test pins are as they were
    assert list(inspect.signature(vec_env.VecOthelloEnv.puct_play).parameters)[1:] == ["evaluate", "simulations", "sample",
                                                                                        "begin_kw"]
    rn = noise.RootNoise()
    assert rn.epsilon == 64 and rn.alpha == 0.3 and rn.table.shape == (4096,)
    assert noise.RootNoise(epsilon=1.0, alpha=1.0).epsilon == 256 and noise.RootNoise(epsilon=0.0).epsilon == 0
    for bad in (-0.1, 1.01):
        with pytest.raises(ValueError):
            noise.RootNoise(epsilon=bad)
