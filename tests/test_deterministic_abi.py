"""CPU: the C ABI of deterministic mode (the *_det entry points and their workspace queries, include/waldo_hip.h
"Reproducible gradients"), its host-side validation, and the Python switch.  No compute call is made here."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "waldo_hip.h")
ENTRY = ("waldo_grid_sample2d_bwd_det", "waldo_grid_sample2d_ex_bwd_det", "waldo_occ_composite_bwd_det",
         "waldo_tps_grid_bwd_det", "waldo_flow_ctx_alpha_bwd_det", "waldo_flow_ctx_warp_bwd_det",
         "waldo_warp_composite_bwd_det")
QUERY = ("waldo_grid_sample2d_bwd_det_workspace_bytes", "waldo_occ_composite_bwd_det_workspace_bytes",
         "waldo_tps_grid_bwd_det_workspace_bytes", "waldo_flow_ctx_alpha_bwd_det_workspace_bytes",
         "waldo_flow_ctx_warp_bwd_det_workspace_bytes", "waldo_warp_composite_bwd_det_workspace_bytes")
FAKE = 256  # a non-null "pointer": every call below must return before anything is launched or dereferenced


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def _msg(lib):
    return lib.waldo_last_error_string().decode()


def r256(b):
    return (b + 255) // 256 * 256


def cdiv(a, b):
    return -(-a // b)


def test_det_entry_points_declared_exported_and_bound(lib):
    from waldo_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(build.LIB)
    for name in ENTRY + QUERY:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(raw, name), name
    for name in ENTRY:
        assert name in _lib.SIGNATURES, name
        # the workspace and its size travel together
        assert re.search(name + r"\s*\([^;]*void\s*\*\s*workspace\s*,\s*int64_t\s+workspace_bytes\b[^;]*\)\s*;", src), name
    for name in QUERY:
        assert name in _lib.PLAIN and name in _lib.DET_QUERIES, name
        assert _lib.PLAIN[name][0] is ctypes.c_int64


def test_abi_version_stays_1020(lib):
    from waldo_amd import _lib
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION


def test_header_states_the_contract():
    text = open(HEADER).read()
    for phrase in ("Reproducible gradients", "OVERWRITTEN", "k = 63 - ex - clog", "SLAB", "FIXED POINT", "ALL NaN",
                   "2^32 contributions"):
        assert phrase in text, phrase


# ---- workspace queries: the header's formulas, and growth with every size they depend on
def _gs_ws(n, nin, c, hi, wi, ho, wo):
    return r256(nin * c * hi * wi * 8) + r256(nin * c * 4)


def _groups(hw):
    return cdiv(cdiv(hw, 256), 4)


def _occ_ws(m, l, hw):
    return r256(m * _groups(hw) * l * l * 4)


def _tps_ws(b, hw, k3):
    return r256(b * cdiv(cdiv(hw, 1024), 4) * k3 * 2 * 4)


def _alpha_ws(b, tw, l, nl, h, w, s):
    n, hwd = b * tw, h * s * w * s
    g = _groups(hwd)
    return (r256(n * l * hwd * 4) if s > 1 else 0) + r256(n * g * l * l * 4) + r256(n * g * (l - 1) * nl * 4)


def _warp_ws(b, tw, tc, tp, l, h, w, s):
    m, hwd = b * tc * tp, h * s * w * s
    g = _groups(hwd)
    return ((r256(m * l * 2 * hwd * 4) if s > 1 else 0) + r256(m * l * hwd * 4) + r256(b * tw * l * hwd * 8)
            + r256(b * tw * l * 4) + r256(m * g * l * l * 4))


def _wc_ws(lib, f, l, h, w, k3):
    return lib.waldo_warp_composite_bwd_workspace_bytes(f, l, h, w, k3) + r256(f * cdiv(h, 16) * cdiv(w, 16) * 4 * l * l * 4)


CASES = (
    ("waldo_grid_sample2d_bwd_det_workspace_bytes", _gs_ws, (6, 3, 4, 32, 48, 64, 96), (1, 2, 3, 4)),
    ("waldo_occ_composite_bwd_det_workspace_bytes", _occ_ws, (12, 9, 128 * 256), (0, 1, 2)),
    ("waldo_tps_grid_bwd_det_workspace_bytes", _tps_ws, (10, 128 * 256, 19), (0, 1, 2)),
    ("waldo_flow_ctx_alpha_bwd_det_workspace_bytes", _alpha_ws, (2, 3, 9, 10, 32, 64, 4), (0, 1, 2, 3, 4, 5, 6)),
    ("waldo_flow_ctx_warp_bwd_det_workspace_bytes", _warp_ws, (2, 3, 2, 3, 9, 32, 64, 4), (0, 1, 2, 3, 4, 5, 6, 7)),
)


@pytest.mark.parametrize("name,formula,base,grows", CASES, ids=[c[0] for c in CASES])
def test_workspace_queries_match_the_header_formula_and_grow(lib, name, formula, base, grows):
    fn = getattr(lib, name)
    assert fn(*base) == formula(*base) > 0
    for i in grows:  # doubling any size the workspace depends on needs more of it
        args = list(base)
        args[i] *= 2
        assert fn(*args) == formula(*args) > fn(*base), (name, i)


def test_warp_composite_det_workspace(lib):
    q = lib.waldo_warp_composite_bwd_det_workspace_bytes
    base = (4, 8, 64, 96, 19)
    assert q(*base) == _wc_ws(lib, *base) > lib.waldo_warp_composite_bwd_workspace_bytes(*base)
    for i in (0, 1, 2, 3):
        args = list(base)
        args[i] *= 2
        assert q(*args) == _wc_ws(lib, *args) > q(*base)
    # no deterministic kernel where the generic backward would run: L > 17, K3 != 19, 4 does not divide W
    assert q(4, 24, 64, 96, 19) == 0 and q(4, 8, 64, 96, 15) == 0 and q(4, 8, 64, 98, 19) == 0
    assert lib.waldo_tps_grid_bwd_det_workspace_bytes(4, 4096, 137) == 0


# ---- rejected before any launch, with a message
def _gs(lib, n=4, nin=4, c=3, hi=16, wi=16, ho=16, wo=16, od=None, inner=None, gi=FAKE, ws=FAKE, nb=1 << 40):
    od = n if od is None else od
    inner = n if inner is None else inner
    return lib.waldo_grid_sample2d_bwd_det(FAKE, FAKE, FAKE, gi, None, n, nin, c, hi, wi, ho, wo, 0.0, od, inner, ws, nb,
                                           None)


def test_grid_sample_det_rejects(lib):
    need = lib.waldo_grid_sample2d_bwd_det_workspace_bytes(4, 4, 3, 16, 16, 16, 16)
    assert _gs(lib, c=-1) == -1 and "bad shape" in _msg(lib)
    assert _gs(lib, nb=need - 1) == -1 and f"{need} needed" in _msg(lib)
    assert _gs(lib, ws=None) == -1 and "workspace" in _msg(lib)
    assert _gs(lib, nin=3) == -1 and "Nin=3" in _msg(lib)
    # one input map read by 8 output maps of 32767 x 32767 pixels: > 2^32 contributions to a texel
    assert _gs(lib, n=8, nin=1, ho=32767, wo=32767, od=8, inner=1) == -1
    assert "2^32 contributions" in _msg(lib)
    assert lib.waldo_grid_sample2d_bwd_det(None, FAKE, FAKE, FAKE, None, 4, 4, 3, 16, 16, 16, 16, 0.0, 4, 4, FAKE,
                                           1 << 40, None) == -1 and "null pointer" in _msg(lib)
    # nothing asked for: nothing to do
    assert _gs(lib, gi=None) == 0
    assert lib.waldo_grid_sample2d_ex_bwd_det(FAKE, FAKE, FAKE, FAKE, None, 4, 4, 3, 16, 16, 16, 16, 0.0, 4, 4, 2, 1, 0,
                                              1.0, 0.0, FAKE, 1 << 40, None) == -1 and "bad gradient slots" in _msg(lib)


def test_occ_and_tps_det_reject(lib):
    occ = lib.waldo_occ_composite_bwd_det
    need = lib.waldo_occ_composite_bwd_det_workspace_bytes(8, 9, 4096)
    assert occ(FAKE, FAKE, FAKE, FAKE, FAKE, 8, 40, 4096, 1, FAKE, 1 << 40, None) == -1 and "bad shape" in _msg(lib)
    assert occ(FAKE, FAKE, FAKE, FAKE, FAKE, 8, 9, -1, 1, FAKE, 1 << 40, None) == -1 and "bad shape" in _msg(lib)
    assert occ(FAKE, FAKE, FAKE, FAKE, FAKE, 8, 9, 4096, 1, FAKE, need - 1, None) == -1 and f"{need} needed" in _msg(lib)
    assert occ(FAKE, FAKE, FAKE, None, FAKE, 8, 9, 4096, 1, FAKE, need, None) == -1 and "null pointer" in _msg(lib)
    tps = lib.waldo_tps_grid_bwd_det
    need = lib.waldo_tps_grid_bwd_det_workspace_bytes(8, 4096, 19)
    assert tps(FAKE, FAKE, FAKE, 8, -4, 19, FAKE, 1 << 40, None) == -1 and "bad shape" in _msg(lib)
    assert tps(FAKE, FAKE, FAKE, 8, 4096, 137, FAKE, 1 << 40, None) == -1 and "K3 <= 136" in _msg(lib)
    assert tps(FAKE, FAKE, FAKE, 8, 4096, 19, FAKE, need - 1, None) == -1 and f"{need} needed" in _msg(lib)
    assert tps(FAKE, FAKE, None, 8, 4096, 19, FAKE, need, None) == -1 and "null pointer" in _msg(lib)


def test_flow_ctx_det_reject(lib):
    alpha = lib.waldo_flow_ctx_alpha_bwd_det
    ptrs = [FAKE] * 9
    need = lib.waldo_flow_ctx_alpha_bwd_det_workspace_bytes(2, 3, 9, 20, 16, 32, 4)
    assert alpha(*ptrs, FAKE, 1 << 40, 2, 4, 3, 9, 20, 23, 3, -16, 32, 4, None) == -1 and "bad shape" in _msg(lib)
    assert alpha(*ptrs, FAKE, 1 << 40, 2, 2, 3, 9, 20, 23, 3, 16, 32, 4, None) == -1 and "frame window" in _msg(lib)
    assert alpha(*ptrs, FAKE, need - 1, 2, 4, 3, 9, 20, 23, 3, 16, 32, 4, None) == -1 and f"{need} needed" in _msg(lib)
    assert alpha(*ptrs, None, 0, 2, 4, 3, 9, 20, 23, 3, 16, 32, 4, None) == -1 and "workspace" in _msg(lib)
    bad = list(ptrs)
    bad[6] = None  # grad_alpha_lr
    assert alpha(*bad, FAKE, need, 2, 4, 3, 9, 20, 23, 3, 16, 32, 4, None) == -1 and "null pointer" in _msg(lib)

    warp = lib.waldo_flow_ctx_warp_bwd_det
    ptrs = [FAKE] * 12
    need = lib.waldo_flow_ctx_warp_bwd_det_workspace_bytes(2, 3, 2, 3, 9, 16, 32, 4)
    assert warp(*ptrs, FAKE, 1 << 40, 2, 4, 3, 2, 3, 40, 16, 32, 4, None) == -1 and "bad shape" in _msg(lib)
    assert warp(*ptrs, FAKE, 1 << 40, 2, 4, 5, 2, 3, 9, 16, 32, 4, None) == -1 and "frame counts" in _msg(lib)
    assert warp(*ptrs, FAKE, need - 1, 2, 4, 3, 2, 3, 9, 16, 32, 4, None) == -1 and f"{need} needed" in _msg(lib)
    bad = list(ptrs)
    bad[9] = None  # grad_flow_lr
    assert warp(*bad, FAKE, need, 2, 4, 3, 2, 3, 9, 16, 32, 4, None) == -1 and "null pointer" in _msg(lib)
    # 3 x 3 units of 32767 x 32767 pixels on one context plane: > 2^32 contributions to a texel
    assert warp(*ptrs, FAKE, 1 << 60, 1, 4, 3, 3, 3, 2, 32767, 32767, 1, None) == -1
    assert "2^32 contributions" in _msg(lib)


@pytest.mark.parametrize("code", [0, 1, 2])
def test_warp_composite_det_rejects(lib, code):
    wc = lib.waldo_warp_composite_bwd_det

    def call(L=8, H=64, W=96, K3=19, F=2, ws=FAKE, nb=1 << 40, gl=FAKE):
        return wc(FAKE, FAKE, FAKE, FAKE, FAKE, None, gl, FAKE, FAKE, ws, nb, F, L, H, W, K3, 0.0, code, None)

    need = lib.waldo_warp_composite_bwd_det_workspace_bytes(2, 8, 64, 96, 19)
    assert call(L=99) == -1 and "unsupported shape" in _msg(lib)
    # the generic backward's shapes have no deterministic kernel -- also at F == 0
    for kw in (dict(L=24), dict(K3=15), dict(W=98)):
        for f in (2, 0):
            assert call(F=f, **kw) == -1 and "no deterministic kernel" in _msg(lib), kw
    assert call(nb=need - 1) == -1 and f"{need} needed" in _msg(lib)
    assert call(ws=None, nb=0) == -1 and "workspace" in _msg(lib)
    assert call(gl=None) == -1 and "null pointer" in _msg(lib)
    assert call(F=0) == 0
    assert wc(*([None] * 10), 0, 2, 8, 64, 96, 19, 0.0, 7, None) == -1 and "unknown dtype" in _msg(lib)


def test_fills_inside_the_det_entry_points_are_kernels():
    """(tests/test_abi.py scans the sources for memset calls; this pins the new header to the same rule)"""
    text = open(os.path.join(ROOT, "waldo_amd", "csrc", "det_common.hip.h")).read()
    assert "hipMemset" not in text and "hipMemcpy" not in text


# ---- the Python switch
@pytest.fixture
def torch_flag():
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def test_mode_is_exported_from_the_package():
    import waldo_amd
    from waldo_amd import functional as WF
    assert waldo_amd.set_deterministic is WF.set_deterministic
    assert waldo_amd.is_deterministic is WF.is_deterministic
    assert waldo_amd.deterministic is WF.deterministic


def test_set_deterministic_three_values(torch_flag):
    from waldo_amd import functional as WF
    try:
        torch.use_deterministic_algorithms(False)
        WF.set_deterministic(None)
        assert WF.is_deterministic() is False  # the default follows torch
        torch.use_deterministic_algorithms(True)
        assert WF.is_deterministic() is True
        WF.set_deterministic(False)  # override, either way
        assert WF.is_deterministic() is False
        torch.use_deterministic_algorithms(False)
        WF.set_deterministic(True)
        assert WF.is_deterministic() is True
        WF.set_deterministic(None)
        assert WF.is_deterministic() is False
        for bad in (1, 0, "on"):
            with pytest.raises(TypeError):
                WF.set_deterministic(bad)
    finally:
        WF.set_deterministic(None)


def test_deterministic_context_nests_and_restores(torch_flag):
    from waldo_amd import functional as WF
    torch.use_deterministic_algorithms(False)
    WF.set_deterministic(None)
    try:
        with WF.deterministic():
            assert WF.is_deterministic()
            with WF.deterministic(False):
                assert not WF.is_deterministic()
                with WF.deterministic(None):
                    assert not WF.is_deterministic()
                    torch.use_deterministic_algorithms(True)
                    assert WF.is_deterministic()
                    torch.use_deterministic_algorithms(False)
                assert not WF.is_deterministic()
            assert WF.is_deterministic()
        assert WF._deterministic is None and not WF.is_deterministic()
        with pytest.raises(KeyError):
            with WF.deterministic(True):
                assert WF.is_deterministic()
                raise KeyError("x")
        assert WF._deterministic is None
        WF.set_deterministic(False)
        ctx = WF.deterministic(True)
        with ctx:
            with ctx:  # the same object, re-entered
                assert WF.is_deterministic()
            assert WF.is_deterministic()
        assert WF._deterministic is False
        with pytest.raises(TypeError):
            WF.deterministic("yes")
    finally:
        WF.set_deterministic(None)
