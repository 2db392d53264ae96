"""CPU: the C ABI of include/waldo_hip.h "LPIPS level distance" as far as it goes without a GPU -- the symbols, the size
queries and the argument checks.  The pointers are never dereferenced: every case is refused before a launch."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 64  # a non-null "pointer"
NAMES = ("waldo_lpips_level_fwd", "waldo_lpips_level_bwd")
QUERIES = ("waldo_lpips_level_workspace_bytes", "waldo_lpips_level_saved_bytes")
FWD_REQUIRED = (0, 1, 2, 3, 5)  # f0, f1, w, out, workspace (saved may be NULL: no backward wanted)


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def fwd(lib, ptrs=(PTR,) * 6, ws=1 << 20, n=2, c=5, p=63):
    return lib.waldo_lpips_level_fwd(*ptrs, ws, n, c, p, 1e-10, None)


def bwd(lib, ptrs=(PTR,) * 6, n=2, c=5, p=63):
    return lib.waldo_lpips_level_bwd(*ptrs, n, c, p, None)


def without(n, i):
    return (PTR,) * i + (None,) + (PTR,) * (n - i - 1)


def test_symbols_are_exported_bound_and_described(lib):
    from waldo_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in QUERIES:
        assert hasattr(lib, name) and name in _lib.PLAIN, name
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * LPIPS level distance:"):]
    for needle in NAMES + QUERIES + ("NO ATOMICS", "EXACT 0", "n0[p] == 0", "AFTER the square root"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


def test_queries_are_monotone_multiples_of_256_and_zero_for_bad_shapes(lib):
    ws, sv = lib.waldo_lpips_level_workspace_bytes, lib.waldo_lpips_level_saved_bytes
    assert ws(1, 1, 1) == 256 and sv(1, 1, 1) == 256
    assert ws(2, 64, 64 * 64) == 2 * 64 * 4                     # one float per tile of 64 pixels
    assert sv(2, 64, 64 * 64) == 2 * 3 * 64 * 64 * 4            # three floats per pixel
    sizes = [(1, 3, 1), (1, 3, 63), (1, 3, 64), (1, 3, 65), (2, 3, 65), (2, 3, 4096), (2, 3, 262144), (3, 3, 262144),
             (8, 3, 262144), (8, 3, 524288), (64, 3, 524288), (64, 3, 1 << 24)]
    for q in (ws, sv):
        got = [q(*s) for s in sizes]
        assert all(v > 0 and v % 256 == 0 for v in got), got
        assert got == sorted(got), got                          # monotone in N and in P, across the tile switch too
        assert q(2, 64, 4096) == q(2, 512, 4096)                # and independent of C
    assert ws(64, 3, 1 << 24) > ws(64, 3, 524288) > ws(1, 3, 1)
    for bad in ((0, 5, 63), (-1, 5, 63), (2, 0, 63), (2, -4, 63), (2, 5, 0), (2, 5, -63),
                (1, 1 << 16, 1 << 15), (1, 2, 1 << 30), (1 << 31, 1, 64)):
        assert ws(*bad) == 0 and sv(*bad) == 0, bad
    assert ws(1, 1, (1 << 31) - 1) > 0 and ws(1, (1 << 31) - 1, 1) > 0  # C P = 2^31 - 1 is the last size served


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
def test_entry_points_reject_bad_arguments_before_any_launch(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.waldo_last_error_string(), (call.__name__, kw, lib.waldo_last_error_string())


def test_null_checks_come_first(lib):
    """A null pointer is reported even where the shape is bad too, a bad shape before its size, and both before the
    workspace."""
    assert fwd(lib, ptrs=without(6, 0), n=0) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert bwd(lib, ptrs=without(6, 5), c=1 << 16, p=1 << 15) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert fwd(lib, n=0, ws=0) == -1 and b"bad shape" in lib.waldo_last_error_string()
    assert fwd(lib, c=0, p=1 << 40) == -1 and b"bad shape" in lib.waldo_last_error_string()
    assert fwd(lib, c=1 << 16, p=1 << 15, ws=0) == -1 and b"too large" in lib.waldo_last_error_string()
