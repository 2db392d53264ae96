"""CPU: the 16-bit WIF path's C ABI (the *_dt entry points, enum waldo_dtype) and the fp32 defaults of its Python
arguments.  No compute call is made here."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "waldo_hip.h")
NEW = ("waldo_flow_ctx_warp_raw_fwd_dt", "waldo_frame_warp_fuse_raw_fwd_dt", "waldo_wif_fuse_fwd_dt",
       "waldo_wif_fuse_bwd_dt")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def test_dt_entry_points_declared_exported_and_bound(lib):
    from waldo_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(build.LIB)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    for code, value in (("WALDO_DTYPE_F32", 0), ("WALDO_DTYPE_F16", 1), ("WALDO_DTYPE_BF16", 2)):
        assert re.search(code + r"\s*=\s*" + str(value), src), code


def test_abi_version_1020(lib):
    from waldo_amd import _lib
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION


def test_unknown_dtype_code_rejected_without_gpu(lib):
    """A dtype code outside enum waldo_dtype: WALDO_EINVAL and a message, before any pointer is looked at."""
    assert lib.waldo_wif_fuse_fwd_dt(None, None, None, 1, 2, 5, 4, 64, 1, 0, 7, None) == -1
    assert b"unknown dtype" in lib.waldo_last_error_string()
    assert lib.waldo_wif_fuse_bwd_dt(*([None] * 6), 1, 2, 5, 4, 64, 1, 3, 0, None) == -1
    assert b"unknown dtype" in lib.waldo_last_error_string()
    args = [None] * 13 + [1, 4, 4, 4, 1, 8, 8, 8, 4, 3, 4]
    assert lib.waldo_flow_ctx_warp_raw_fwd_dt(*args, -1, None) == -1
    assert b"unknown raw dtype" in lib.waldo_last_error_string()
    args = [None] * 7 + [1, 4, 4, 1, 3, 8, 32, 32, 0]
    assert lib.waldo_frame_warp_fuse_raw_fwd_dt(*args, 1e-6, 5, None) == -1
    assert b"unknown raw dtype" in lib.waldo_last_error_string()
    # a known code still gets today's validation (a null score here)
    assert lib.waldo_frame_warp_fuse_raw_fwd_dt(*args, 1e-6, 2, None) == -1
    assert b"null pointer" in lib.waldo_last_error_string()


def test_python_defaults_are_fp32():
    import torch
    from waldo_amd import functional as WF
    from waldo_amd.nets import lvd
    from waldo_amd.tools import demo
    assert inspect.signature(lvd.decode_output).parameters["raw_dtype"].default is None
    assert inspect.signature(WF.flow_ctx_warp_into_raw).parameters["raw_dtype"].default == torch.float32
    for fn in (demo.predict, demo.decode_units, demo.predict_sharded, demo._decode_block, demo.run):
        assert inspect.signature(fn).parameters["raw_dtype"].default is None, fn.__name__
    assert lvd._raw_dtype(None) == torch.float32
    with pytest.raises(ValueError):
        lvd._raw_dtype(torch.float64)
