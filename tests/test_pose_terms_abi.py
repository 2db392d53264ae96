"""CPU: the C ABI of include/waldo_hip.h "Pose objective" as far as it goes without a GPU -- the symbols, the workspace
query and the argument checks.  The pointers are never dereferenced: every case is refused before a launch."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 64  # a non-null "pointer"
NAMES = ("waldo_pose_l1_fwd", "waldo_pose_l1_bwd")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def fwd(lib, ptrs=(P,) * 10, ws=1 << 20, f=6, e=(24, 12, 3)):
    return lib.waldo_pose_l1_fwd(*ptrs, ws, f, *e, None)


def bwd(lib, ptrs=(P,) * 17, f=6, e=(24, 12, 3)):
    return lib.waldo_pose_l1_bwd(*ptrs, f, *e, None)


def without(n, i):
    return (P,) * i + (None,) + (P,) * (n - i - 1)


def test_symbols_are_exported_bound_and_described(lib):
    from waldo_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert hasattr(lib, "waldo_pose_l1_workspace_bytes") and "waldo_pose_l1_workspace_bytes" in _lib.PLAIN
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Pose objective:"):]
    for needle in NAMES + ("waldo_pose_l1_workspace_bytes", "NO ATOMICS", "EXACT 0", "sgn(0) = 0"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


def test_workspace_query_grows_with_the_sizes(lib):
    q = lib.waldo_pose_l1_workspace_bytes
    small = q(6, 24, 12, 3)                    # one workgroup per term
    assert small == 256 and small % 256 == 0
    recipe = q(56, 512, 256, 16)               # 14 + 7 + 1 workgroups of 2048 elements
    assert recipe == 256
    large = q(256, 3968, 16, 31)               # 496 + 2 + 4 partials
    assert large == (502 * 4 + 255) // 256 * 256
    assert q(512, 3968, 16, 31) > large > small
    assert q(256, 3968, 4096, 31) > large
    assert q(256, 3968, 16, 4096) > large
    for bad in ((0, 24, 12, 3), (-1, 24, 12, 3), (6, 0, 12, 3), (6, 24, -1, 3), (6, 24, 12, 0),
                (1 << 25, 1, 1, 1), (1 << 20, 1 << 12, 1, 1)):
        assert q(*bad) == 0, bad


@pytest.mark.parametrize("call,kw,msg", [
    (fwd, dict(f=0), b"bad shape"), (fwd, dict(f=-3), b"bad shape"), (fwd, dict(e=(0, 12, 3)), b"bad shape"),
    (fwd, dict(e=(24, -1, 3)), b"bad shape"), (fwd, dict(e=(24, 12, 0)), b"bad shape"),
    (fwd, dict(f=1 << 25, e=(1, 1, 1)), b"too large"), (fwd, dict(f=1 << 20, e=(1 << 12, 1, 1)), b"too large"),
    (fwd, dict(ws=255), b"workspace"), (fwd, dict(ws=0), b"workspace"),
    (fwd, dict(f=256, e=(3968, 16, 31), ws=2047), b"workspace"),
    (bwd, dict(f=0), b"bad shape"), (bwd, dict(e=(24, 12, 0)), b"bad shape"),
    (bwd, dict(f=1 << 20, e=(1, 1 << 12, 1)), b"too large"),
] + [(fwd, dict(ptrs=without(10, i)), b"null pointer") for i in range(10)]
  + [(bwd, dict(ptrs=without(17, i)), b"null pointer") for i in (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13)])
def test_entry_points_reject_bad_arguments_before_any_launch(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.waldo_last_error_string(), (call.__name__, kw, lib.waldo_last_error_string())


def test_null_checks_come_first(lib):
    """A null pointer is reported even where the shape is bad too, and a bad shape before the workspace."""
    assert fwd(lib, ptrs=without(10, 0), f=0) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert fwd(lib, f=0, ws=0) == -1 and b"bad shape" in lib.waldo_last_error_string()
