"""CPU: the C ABI of include/waldo_hip.h "Optimizer step" as far as it goes without a GPU -- the symbols, the limits, the
workspace query and the argument checks.  The device pointers are never dereferenced: every case is refused before a
launch; the host arrays are real."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 64  # a non-null, 16-byte aligned "device pointer"
NAMES = ("waldo_adam_limits", "waldo_adam_workspace_bytes", "waldo_adam_step")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def i64s(values):
    return (ctypes.c_int64 * max(len(values), 1))(*values)


def ptrs(values):
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def step(lib, numels=(5, 4096), p=None, g=None, m=None, v=None, wd=None, n=None, state=PTR, hyper=PTR, loss=None,
         ws=PTR, ws_bytes=1 << 20, arrays=(True,) * 5):
    k = len(numels)
    a = [ptrs(list(x) if x is not None else [PTR] * k) for x in (p, g, m, v)] + [i64s(list(numels))]
    a = [x if keep else None for x, keep in zip(a, arrays)]
    decays = None if wd is None else (ctypes.c_float * max(k, 1))(*wd)
    launches = ctypes.c_int(-1)
    rc = lib.waldo_adam_step(*a, decays, k if n is None else n, state, hyper, loss, ws, ws_bytes, 0, ctypes.byref(launches),
                             None)
    assert launches.value == 0      # nothing was launched
    return rc


def test_symbols_are_declared_exported_and_bound(lib):
    from waldo_amd import _lib
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Optimizer step (waldo_amd.optim)"):]
    for name in NAMES:
        assert hasattr(lib, name) and (name in _lib.SIGNATURES or name in _lib.PLAIN) and name in sec, name
    for needle in ("NO ATOMICS", "BY VALUE", "2 ceil(n / K) + 1", "WALDO_ADAM_STATE_WORDS 16", "WALDO_ADAM_HYPER_WORDS 12",
                   "null pointer", "bad shape", "too large", "not aligned", "workspace"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


def test_limits(lib):
    from waldo_amd import optim
    out = (ctypes.c_int * 4)()
    assert lib.waldo_adam_limits(out, 4) == 4 and lib.waldo_adam_limits(None, 0) == 4
    k, chunk, state_words, hyper_words = out
    assert 1 <= k and k * 48 < 4096                 # the pack travels in the kernel arguments
    assert chunk % 1024 == 0                        # whole 16-byte loads of a 256-thread workgroup
    assert (state_words, hyper_words) == (optim.STATE_WORDS, optim.HYPER_WORDS) == (16, 12)
    two = (ctypes.c_int * 4)(-1, -1, -1, -1)
    assert lib.waldo_adam_limits(two, 2) == 4 and list(two) == [k, chunk, -1, -1]
    assert optim.limits() == dict(tensors_per_launch=k, chunk=chunk, state_words=16, hyper_words=12)
    assert optim.launches_per_step(0) == 1 and optim.launches_per_step(k) == 3 and optim.launches_per_step(k + 1) == 5


def test_workspace_query(lib):
    q = lib.waldo_adam_workspace_bytes
    out = (ctypes.c_int * 2)()
    lib.waldo_adam_limits(out, 2)
    chunk = out[1]
    assert q(0, None) == 256 and q(1, i64s([0])) == 256 and q(1, i64s([1])) == 256
    assert q(1, i64s([32 * chunk])) == 256 and q(1, i64s([32 * chunk + 1])) == 512      # 8 bytes per chunk
    assert q(3, i64s([chunk, chunk + 1, 0])) == 256
    assert q(2, i64s([1000 * chunk, 24 * chunk])) == 8 * 1024
    sizes = [[1], [chunk], [chunk + 1] * 40, [chunk * 100] * 7, [1 << 33], [1 << 33, 1 << 33]]
    got = [q(len(s), i64s(s)) for s in sizes]
    assert all(v > 0 and v % 256 == 0 for v in got) and got == sorted(got), got
    # bad sizes: a negative count or size, no array, too many chunks in one tensor or in all
    assert q(-1, i64s([1])) == 0 and q(1, None) == 0 and q(2, i64s([5, -1])) == 0
    last = ((1 << 31) - 1) * chunk
    assert q(1, i64s([last])) > 0 and q(1, i64s([last + 1])) == 0 and q(2, i64s([last, 1])) == 0
    assert q(1, i64s([(1 << 63) - 1])) == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(state=None), b"null pointer"), (dict(hyper=None), b"null pointer"), (dict(ws=None), b"null pointer"),
    (dict(arrays=(False, True, True, True, True)), b"null pointer"), (dict(arrays=(True, False, True, True, True)), b"null pointer"),
    (dict(arrays=(True, True, False, True, True)), b"null pointer"), (dict(arrays=(True, True, True, False, True)), b"null pointer"),
    (dict(arrays=(True, True, True, True, False)), b"null pointer"),
    (dict(p=[PTR, None]), b"null pointer"), (dict(g=[None, PTR]), b"null pointer"), (dict(m=[PTR, None]), b"null pointer"),
    (dict(v=[None, PTR]), b"null pointer"),
    (dict(n=-1), b"bad shape"), (dict(numels=(5, -1)), b"bad shape"), (dict(numels=(-4096,)), b"bad shape"),
    (dict(numels=(1 << 62,)), b"too large"), (dict(numels=(((1 << 31) - 1) * 4096, 1)), b"too large"),
    (dict(p=[PTR + 2, PTR]), b"not aligned"), (dict(g=[PTR, PTR + 1]), b"not aligned"), (dict(m=[PTR + 3, PTR]), b"not aligned"),
    (dict(v=[PTR, PTR + 2]), b"not aligned"), (dict(state=PTR + 2), b"not aligned"), (dict(hyper=PTR + 1), b"not aligned"),
    (dict(loss=PTR + 2), b"not aligned"), (dict(ws=PTR + 4), b"not aligned"),
    (dict(ws_bytes=255), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws_bytes=-1), b"workspace"),
    (dict(numels=(4096 * 32 + 1,), ws_bytes=511), b"workspace"),
])
def test_step_refuses_bad_arguments_before_any_launch(lib, kw, msg):
    assert step(lib, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


def test_order_of_the_checks_and_what_is_allowed(lib):
    """A null pointer is reported before a bad shape, a bad shape before a size, both before an alignment and the
    workspace; the buffers of an EMPTY tensor are not looked at."""
    assert step(lib, state=None, numels=(5, -1)) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert step(lib, numels=(1 << 62, -1)) == -1 and b"bad shape" in lib.waldo_last_error_string()
    assert step(lib, numels=(1 << 62, 5), p=[PTR + 1, PTR]) == -1 and b"too large" in lib.waldo_last_error_string()
    assert step(lib, p=[PTR + 1, PTR], ws_bytes=0) == -1 and b"not aligned" in lib.waldo_last_error_string()
    # (an empty tensor's null / odd pointers pass the checks: what is refused here is the workspace, the last check)
    assert step(lib, numels=(0, 5), p=[None, PTR], g=[PTR + 1, PTR], ws_bytes=0) == -1
    assert b"workspace" in lib.waldo_last_error_string()
    assert step(lib, numels=(0, 5), p=[PTR, None], ws_bytes=0) == -1 and b"null pointer" in lib.waldo_last_error_string()
