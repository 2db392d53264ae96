"""CPU: the C ABI of include/waldo_hip.h "LPIPS level distance in 16 bits" as far as it goes without a GPU -- the
symbols and the argument checks of the ``_dt`` entry points.  The pointers are never dereferenced: every case is refused
before a launch.  The bad arguments are tests/test_lpips_abi.py's own table, sent through the ``_dt`` entries with
either 16-bit code: the same messages in the same order.  (The 16-bit form keeps the fp32 kernels' tile, so there are
no ``_dt`` size queries: the fp32 ones serve both.)"""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 64  # a non-null "pointer"
F32, F16, BF16 = 0, 1, 2  # include/waldo_hip.h: enum waldo_dtype
NAMES = ("waldo_lpips_level_fwd_dt", "waldo_lpips_level_bwd_dt")
FWD_REQUIRED = (0, 1, 2, 3, 5)  # f0, f1, w, out, workspace (saved may be NULL: no backward wanted)


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def fwd(lib, ptrs=(PTR,) * 6, ws=1 << 20, n=2, c=5, p=63, dtype=BF16):
    return lib.waldo_lpips_level_fwd_dt(*ptrs, ws, n, c, p, 1e-10, dtype, None)


def bwd(lib, ptrs=(PTR,) * 6, n=2, c=5, p=63, dtype=BF16):
    return lib.waldo_lpips_level_bwd_dt(*ptrs, n, c, p, dtype, None)


def without(n, i):
    return (PTR,) * i + (None,) + (PTR,) * (n - i - 1)


def test_symbols_are_exported_bound_and_described(lib):
    from waldo_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    assert header.index("WALDO_DTYPE_F32 = 0") < header.index("WALDO_DTYPE_F16 = 1") < header.index("WALDO_DTYPE_BF16 = 2")
    sec = header[header.index(" * LPIPS level distance in 16 bits:"):]
    sec = sec[:sec.index("Clip augmentation")]
    for needle in NAMES + ("WALDO_DTYPE_BF16", "WALDO_DTYPE_F16", "NO ATOMICS", "EXACT 0", "n0[p] == 0",
                           "AFTER the square root", "2-byte alignment", "even P", "nearest-even", "subnormals",
                           "SCALED LOSS", "unknown dtype", "waldo_lpips_level_workspace_bytes"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged
    assert not hasattr(lib, "waldo_lpips_level_workspace_bytes_dt")  # one tile width: the fp32 query serves both


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("call,kw,msg", [
    (fwd, dict(n=0), b"bad shape"), (fwd, dict(n=-2), b"bad shape"), (fwd, dict(c=0), b"bad shape"),
    (fwd, dict(c=-1), b"bad shape"), (fwd, dict(p=0), b"bad shape"), (fwd, dict(p=-63), b"bad shape"),
    (fwd, dict(c=1 << 16, p=1 << 15), b"too large"), (fwd, dict(c=2, p=1 << 30), b"too large"),
    (fwd, dict(n=1 << 31, c=1, p=64), b"too large"),
    (fwd, dict(ws=255), b"workspace"), (fwd, dict(ws=0), b"workspace"), (fwd, dict(ws=-1), b"workspace"),
    (fwd, dict(n=8, c=64, p=524288, ws=8 * 8192 * 4 - 1), b"workspace"),
    (bwd, dict(n=0), b"bad shape"), (bwd, dict(c=0), b"bad shape"), (bwd, dict(p=-1), b"bad shape"),
    (bwd, dict(c=1 << 16, p=1 << 15), b"too large"), (bwd, dict(n=1 << 31, c=1, p=64), b"too large"),
] + [(fwd, dict(ptrs=without(6, i)), b"null pointer") for i in FWD_REQUIRED]
  + [(bwd, dict(ptrs=without(6, i)), b"null pointer") for i in range(6)])
def test_entry_points_reject_bad_arguments_before_any_launch(lib, call, kw, msg, dtype):
    assert call(lib, dtype=dtype, **kw) == -1, (call.__name__, kw)
    err = lib.waldo_last_error_string()
    assert msg in err and (call.__name__ + "_dt").encode() in err, (call.__name__, kw, err)


def test_null_checks_come_first(lib):
    """A null pointer is reported even where the shape is bad too, a bad shape before its size, and both before the
    workspace: the fp32 entry points' order."""
    assert fwd(lib, ptrs=without(6, 0), n=0) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert bwd(lib, ptrs=without(6, 5), c=1 << 16, p=1 << 15) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert fwd(lib, n=0, ws=0) == -1 and b"bad shape" in lib.waldo_last_error_string()
    assert fwd(lib, c=0, p=1 << 40) == -1 and b"bad shape" in lib.waldo_last_error_string()
    assert fwd(lib, c=1 << 16, p=1 << 15, ws=0) == -1 and b"too large" in lib.waldo_last_error_string()


def test_the_fp32_code_is_refused_with_the_fp32_entry_point_named(lib):
    assert fwd(lib, dtype=F32) == -1
    err = lib.waldo_last_error_string()
    assert b"WALDO_DTYPE_F32" in err and b"waldo_lpips_level_fwd" in err.replace(b"waldo_lpips_level_fwd_dt", b""), err
    assert bwd(lib, dtype=F32) == -1
    err = lib.waldo_last_error_string()
    assert b"WALDO_DTYPE_F32" in err and b"waldo_lpips_level_bwd" in err.replace(b"waldo_lpips_level_bwd_dt", b""), err


@pytest.mark.parametrize("code", [3, -1, 7, 1 << 20])
def test_an_unknown_dtype_code_is_refused(lib, code):
    for call in (fwd, bwd):
        assert call(lib, dtype=code) == -1
        assert b"unknown dtype" in lib.waldo_last_error_string(), (call.__name__, code, lib.waldo_last_error_string())
