"""CPU: the C ABI of the 16-bit layer stack of the fused warp/composite (waldo_warp_composite_*_dt) and its host-side
validation.  No compute call is made here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "waldo_hip.h")
NEW = ("waldo_warp_composite_fwd_dt", "waldo_warp_composite_pts_fwd_dt", "waldo_warp_composite_bwd_dt")
F32, F16, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def _fwd(lib, L, H, W, K3, code, F=1):
    return lib.waldo_warp_composite_fwd_dt(*([None] * 6), F, L, H, W, K3, 0.0, code, None)


def _pts(lib, L, H, W, N, code, F=1):
    return lib.waldo_warp_composite_pts_fwd_dt(*([None] * 7), F, L, H, W, N, 0.0, code, None)


def _bwd(lib, L, H, W, K3, code, F=1, ws=None, ws_bytes=0):
    return lib.waldo_warp_composite_bwd_dt(*([None] * 9), ws, ws_bytes, F, L, H, W, K3, 0.0, code, None)


def _msg(lib):
    return lib.waldo_last_error_string().decode()


def test_layers16_entry_points_declared_exported_and_bound(lib):
    from waldo_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(build.LIB)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        # the dtype code is the last argument before the stream
        assert _lib.SIGNATURES[name][-2:] == [ctypes.c_int, ctypes.c_void_p], name
        assert re.search(name + r"\s*\([^;]*int\s+layers_dtype\s*,\s*waldo_stream_t\s+stream\s*\)\s*;", src), name


def test_abi_version_stays_1020(lib):
    from waldo_amd import _lib
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION


@pytest.mark.parametrize("code", [-1, 3, 7])
def test_unknown_dtype_rejected_before_pointers(lib, code):
    assert _fwd(lib, 8, 16, 16, 19, code) == -1
    assert "unknown dtype" in _msg(lib)
    assert _pts(lib, 8, 16, 16, 16, code) == -1
    assert "unknown dtype" in _msg(lib)
    assert _bwd(lib, 8, 16, 16, 19, code) == -1
    assert "unknown dtype" in _msg(lib)


def test_f32_code_keeps_the_fp32_validation(lib):
    """WALDO_DTYPE_F32 is the fp32 entry point: the generic shapes pass to the null-pointer check."""
    assert _fwd(lib, 8, 16, 18, 19, F32) == -1
    assert "null pointer" in _msg(lib)
    assert _bwd(lib, 24, 16, 16, 19, F32) == -1
    assert "null pointer" in _msg(lib)
    assert _fwd(lib, 99, 16, 16, 19, F32) == -1
    assert "unsupported shape" in _msg(lib)
    assert _fwd(lib, 8, 16, 16, 19, F32, F=0) == 0


@pytest.mark.parametrize("code", [F16, BF16])
def test_16bit_unserved_shapes_rejected_with_reason(lib, code):
    # W % 4 != 0: no staged forward, no two-kernel backward
    assert _fwd(lib, 8, 40, 70, 19, code) == -1
    assert "staged forward" in _msg(lib)
    assert _pts(lib, 8, 40, 70, 16, code) == -1
    assert "not served" in _msg(lib)
    assert _bwd(lib, 8, 40, 70, 19, code) == -1
    assert "two-kernel backward" in _msg(lib)
    # K3 != 19 (4 x 3 control points + 3)
    assert _fwd(lib, 8, 16, 16, 15, code) == -1
    assert "staged forward" in _msg(lib)
    # L = 18: the forward is served, the backward is not -- rejected even at F == 0
    assert _fwd(lib, 18, 16, 16, 19, code) == -1
    assert "null pointer" in _msg(lib)
    for f in (1, 0):
        assert _bwd(lib, 18, 16, 16, 19, code, F=f) == -1
        assert "two-kernel backward" in _msg(lib) and "L=18" in _msg(lib)


@pytest.mark.parametrize("code", [F16, BF16])
def test_16bit_served_shapes_pass_to_pointer_checks(lib, code):
    assert _fwd(lib, 8, 16, 16, 19, code, F=0) == 0
    assert _bwd(lib, 17, 16, 16, 19, code, F=0) == 0
    assert _pts(lib, 8, 16, 16, 16, code, F=0) == 0
    assert _bwd(lib, 17, 16, 16, 19, code) == -1
    assert "null pointer" in _msg(lib)


def test_16bit_rejected_under_debug_options(lib):
    from waldo_amd import _lib
    try:
        assert lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 1) == 0
        assert _fwd(lib, 8, 16, 16, 19, BF16) == -1
        assert "staged forward" in _msg(lib)
        assert _fwd(lib, 8, 16, 16, 19, F32) == -1
        assert "null pointer" in _msg(lib)
    finally:
        lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 0)
    try:
        assert lib.waldo_set_debug_option(_lib.DEBUG_BWD_GENERIC, 1) == 0
        assert _bwd(lib, 8, 16, 16, 19, F16) == -1
        assert "two-kernel backward" in _msg(lib)
    finally:
        lib.waldo_set_debug_option(_lib.DEBUG_BWD_GENERIC, 0)


def test_python_layers16_dispatch():
    """functional.warp_composite serves a 16-bit stack on its own kernels only where both queries say so."""
    import torch
    from waldo_amd import functional as WF
    pts = torch.zeros(8 * 4, 16, 2)
    for shape, grad, want in (((4, 8, 4, 64, 64), True, True), ((4, 8, 4, 40, 70), False, False),
                              ((4, 24, 4, 64, 64), False, True), ((4, 24, 4, 64, 64), True, False),
                              ((4, 17, 4, 64, 64), True, True)):
        layers = torch.zeros(shape, dtype=torch.bfloat16)
        assert WF._layers16_served(layers, pts, grad) == want, (shape, grad)
    assert not WF._layers16_served(torch.zeros(4, 8, 4, 64, 64, dtype=torch.float16), torch.zeros(32, 9, 2), False)
