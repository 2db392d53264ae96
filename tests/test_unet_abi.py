"""CPU: the C ABI of the plane norm (include/waldo_hip.h "Plane norm": waldo_plane_norm_gelu_fwd / _bwd, the workspace and
limits queries).  No kernel is launched and no GPU is touched: every case is refused, or returns, on the host before a
launch; the pointers are small integers that are never dereferenced."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("waldo_plane_norm_gelu_fwd", "waldo_plane_norm_gelu_bwd", "waldo_plane_norm_workspace_bytes",
         "waldo_plane_norm_limits")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def fwd(lib, x=16, xs=(512, 64), gamma=16, beta=16, eps=1e-5, skip=16, ss=(192, 64), out=16, os_n=704, mean=16, rstd=16,
        ws=None, ws_bytes=0, n=1, c=8, cs=3, h=8, w=8):
    """waldo_plane_norm_gelu_fwd with one argument off."""
    return lib.waldo_plane_norm_gelu_fwd(x, *xs, gamma, beta, eps, skip, *ss, out, os_n, mean, rstd, ws, ws_bytes, n, c, cs,
                                         h, w, None)


def bwd(lib, x=16, xs=(512, 64), gamma=16, beta=16, mean=16, rstd=16, go=16, gs=(704, 64), gx=16, sums=16, ws=None,
        ws_bytes=0, n=1, c=8, h=8, w=8):
    return lib.waldo_plane_norm_gelu_bwd(x, *xs, gamma, beta, mean, rstd, go, *gs, gx, sums, ws, ws_bytes, n, c, h, w, None)


def test_symbols_are_exported_and_bound(lib):
    from waldo_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name), name
    for name, nargs in (("waldo_plane_norm_gelu_fwd", 21), ("waldo_plane_norm_gelu_bwd", 19)):
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][-1] is ctypes.c_void_p
        assert len(_lib.SIGNATURES[name]) == nargs
    assert "waldo_plane_norm_workspace_bytes" in _lib.PLAIN and "waldo_plane_norm_limits" in _lib.PLAIN
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Plane norm:"):]
    for needle in NAMES + ("rstd = 1 / sqrt(var + eps)", "0.5 z (1 + erf(z / sqrt 2))", "NEVER E[x^2] - E[x]^2",
                           "gelu'(z) = Phi(z) + z phi(z)", "NO FLOAT ATOMICS", "the bits of skip"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


def test_the_new_kernels_live_in_a_file_of_their_own():
    from waldo_amd import build
    assert os.path.join(build.CSRC, "plane_norm.hip") in build.sources()


def test_limits_are_ascending_and_the_workspace_follows_the_last(lib):
    from waldo_amd import functional as WF
    lim = WF.plane_norm_limits()
    assert len(lim) >= 2 and lim == sorted(set(lim)) and lim[0] >= 1
    buf = (ctypes.c_int * 1)()
    assert lib.waldo_plane_norm_limits(buf, 1) == len(lim) and buf[0] == lim[0]  # (writes no more than asked)
    assert lib.waldo_plane_norm_limits(None, 0) == len(lim)
    top = lim[-1]
    assert lib.waldo_plane_norm_workspace_bytes(3, 5, 1, top) == 0          # a resident plane needs none
    assert lib.waldo_plane_norm_workspace_bytes(3, 5, 1, top + 1) == 3 * 5 * 2 * 2 * 4   # two chunks, two floats each
    assert lib.waldo_plane_norm_workspace_bytes(3, 5, 3, top) == 3 * 5 * 3 * 2 * 4
    assert lib.waldo_plane_norm_workspace_bytes(0, 5, 3, top) == 0
    assert lib.waldo_plane_norm_workspace_bytes(3, 0, 3, 3) == -1 and b"bad shape" in lib.waldo_last_error_string()
    assert lib.waldo_plane_norm_workspace_bytes(1, 1, 32768, 32769) == -1
    assert b"too large" in lib.waldo_last_error_string()


@pytest.mark.parametrize("kw,msg", [
    (dict(n=-1), b"bad shape"), (dict(c=0), b"bad shape"), (dict(c=-2), b"bad shape"), (dict(cs=-1), b"bad shape"),
    (dict(h=0), b"bad shape"), (dict(w=0), b"bad shape"), (dict(h=-8), b"bad shape"),
    (dict(xs=(-512, 64)), b"negative stride"), (dict(xs=(512, -64)), b"negative stride"),
    (dict(ss=(-192, 64)), b"negative stride"), (dict(ss=(192, -64)), b"negative stride"),
    (dict(os_n=-704), b"negative stride"),
    (dict(os_n=703), b"bad stride"), (dict(os_n=0), b"bad stride"),
    (dict(eps=-1e-5), b"bad eps"), (dict(eps=float("nan")), b"bad eps"), (dict(eps=float("inf")), b"bad eps"),
    (dict(x=None), b"null pointer"), (dict(gamma=None), b"null pointer"), (dict(beta=None), b"null pointer"),
    (dict(out=None), b"null pointer"), (dict(mean=None), b"null pointer"), (dict(rstd=None), b"null pointer"),
    (dict(skip=None), b"null pointer"),                       # Cs > 0 needs a skip
    (dict(x=18), b"not aligned"), (dict(x=17), b"not aligned"), (dict(out=6), b"not aligned"),
    (dict(skip=3), b"not aligned"), (dict(gamma=2), b"not aligned"), (dict(mean=5), b"not aligned"),
    (dict(h=32768, w=32769), b"too large"),                   # H W beyond 2^30
    (dict(n=2 ** 31), b"too large"),
    (dict(n=2 ** 28, c=8), b"too large"),                     # N C planes: a grid of 2^31
    (dict(n=2 ** 20, c=64, h=1024, w=1024, os_n=67 * 2 ** 20), b"too large"),  # 2^26 planes of 128 chunks
    (dict(h=128, w=128, os_n=11 * 128 * 128), b"workspace too small"),   # two chunks per plane and no workspace
    (dict(h=128, w=128, os_n=11 * 128 * 128, ws=16, ws_bytes=8 * 2 * 2 * 4 - 4), b"workspace too small"),
])
def test_fwd_rejects_bad_arguments(lib, kw, msg):
    assert fwd(lib, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


@pytest.mark.parametrize("kw,msg", [
    (dict(n=-1), b"bad shape"), (dict(c=0), b"bad shape"), (dict(h=0), b"bad shape"), (dict(w=-1), b"bad shape"),
    (dict(xs=(-512, 64)), b"negative stride"), (dict(xs=(512, -64)), b"negative stride"),
    (dict(gs=(-704, 64)), b"negative stride"), (dict(gs=(704, -64)), b"negative stride"),
    (dict(x=None), b"null pointer"), (dict(gamma=None), b"null pointer"), (dict(beta=None), b"null pointer"),
    (dict(mean=None), b"null pointer"), (dict(rstd=None), b"null pointer"), (dict(go=None), b"null pointer"),
    (dict(gx=None), b"null pointer"), (dict(sums=None), b"null pointer"),
    (dict(go=18), b"not aligned"), (dict(gx=1), b"not aligned"), (dict(sums=6), b"not aligned"),
    (dict(x=2), b"not aligned"),
    (dict(h=32768, w=32769), b"too large"), (dict(n=2 ** 31), b"too large"), (dict(n=2 ** 28, c=8), b"too large"),
    (dict(h=128, w=128), b"workspace too small"),
    (dict(h=128, w=128, ws=16, ws_bytes=100), b"workspace too small"),
])
def test_bwd_rejects_bad_arguments(lib, kw, msg):
    assert bwd(lib, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


def test_empty_batch_returns_ok_without_a_launch(lib):
    assert fwd(lib, n=0, x=None, gamma=None, beta=None, skip=None, out=None, mean=None, rstd=None) == 0
    assert fwd(lib, n=0, x=None, gamma=None, beta=None, skip=None, out=None, mean=None, rstd=None, cs=0, os_n=512) == 0
    assert bwd(lib, n=0, x=None, gamma=None, beta=None, mean=None, rstd=None, go=None, gx=None, sums=None) == 0


def test_python_surface_checks_shapes_before_anything_else():
    import torch
    from waldo_amd import functional as WF
    x, g = torch.zeros(2, 3, 4, 4), torch.ones(3)
    with pytest.raises(ValueError, match="N, C, H, W"):
        WF.plane_norm_gelu(torch.zeros(3, 4, 4), g, g)
    with pytest.raises(ValueError, match="weight and bias"):
        WF.plane_norm_gelu(x, torch.ones(4), g)
    with pytest.raises(ValueError, match="skip must be"):
        WF.plane_norm_gelu(x, g, g, skip=torch.zeros(2, 1, 4, 5))
    with pytest.raises(ValueError, match="skip must be"):
        WF.plane_norm_gelu(x, g, g, skip=torch.zeros(1, 1, 4, 4))
