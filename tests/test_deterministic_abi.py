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


# ---- characterisation: every refusal and every early return of the ten backward entry points that come in an atomic and
# a deterministic form, pinned to the exact (return code, message).  A row is (keyword overrides of the op's default call,
# return code, message without its "<entry point>: " prefix); the default call itself is valid, so it is never made.
# Rows with two faults pin which one is reported: the entry points do not all agree, and each keeps its own order.
BIG = 1 << 40


def _gs_args(name, inp=FAKE, grid=FAKE, go=FAKE, gi=FAKE, gg=FAKE, n=4, nin=4, c=3, hi=16, wi=16, ho=16, wo=16, od=None,
             inner=None, slots=(4, 4, 0), ws=FAKE, nb=BIG):
    od = max(n, 1) if od is None else od
    inner = max(n, 1) if inner is None else inner
    args = [inp, grid, go, gi, gg, n] + ([nin] if name.endswith("_det") else []) + [c, hi, wi, ho, wo, 0.0, od, inner]
    if "_ex_" in name:
        args += [*slots, 1.0, 0.0]
    return args + ([ws, nb] if name.endswith("_det") else []) + [None]


def _occ_args(name, alpha=FAKE, occ=FAKE, go=FAKE, ga=FAKE, gocc=FAKE, m=8, l=9, hw=4096, div=1, ws=FAKE, nb=BIG):
    return [alpha, occ, go, ga, gocc, m, l, hw, div] + ([ws, nb] if name.endswith("_det") else []) + [None]


def _tps_args(name, basis=FAKE, gg=FAKE, gm=FAKE, b=8, hw=4096, k3=19, ws=FAKE, nb=BIG):
    return [basis, gg, gm, b, hw, k3] + ([ws, nb] if name.endswith("_det") else []) + [None]


def _alpha_args(name, alpha_lr=FAKE, inp=FAKE, dist=FAKE, occ=FAKE, g_a01=FAKE, g_out=FAKE, g_lr=FAKE, g_dist=FAKE,
                g_occ=FAKE, ws=FAKE, nb=BIG, b=2, t=4, tw=3, l=9, nl=20, c=23, off=3, h=16, w=32, s=4):
    return ([alpha_lr, inp, dist, occ, g_a01, g_out, g_lr, g_dist, g_occ, ws] + ([nb] if name.endswith("_det") else [])
            + [b, t, tw, l, nl, c, off, h, w, s, None])


def _warp_args(name, flow_lr=FAKE, isobj=FAKE, a01=FAKE, ctx_ts=FAKE, pred_ts=FAKE, occ=FAKE, g_flow=FAKE, g_ctx=FAKE,
               g_dis=FAKE, g_lr=FAKE, g_a01=FAKE, g_occ=FAKE, ws=FAKE, nb=BIG, b=2, t=4, tw=3, tc=2, tp=3, l=9, h=16,
               w=32, s=4):
    return ([flow_lr, isobj, a01, ctx_ts, pred_ts, occ, g_flow, g_ctx, g_dis, g_lr, g_a01, g_occ, ws]
            + ([nb] if name.endswith("_det") else []) + [b, t, tw, tc, tp, l, h, w, s, None])


_GS_NONE = dict(inp=None, grid=None, go=None, gi=None, gg=None)
_GS_SHAPE = "bad shape N=4 C=-1 in=16x16 out=16x16 outer_div=4 inner=4"
_GS_SLOTS = "bad gradient slots (group 2, stride 1, offset 0)"
_GS_NEED = r256(4 * 3 * 16 * 16 * 8) + r256(4 * 3 * 4)
_GS_OVER = ("a texel of grad_input may receive more than 2^32 contributions (N=%d Ho=%d Wo=%d): no deterministic sum for "
            "this shape")
GS_ATOMIC = (
    (dict(c=-1), -1, _GS_SHAPE),
    (dict(hi=32768, wi=32768), -1, "problem too large for one launch"),
    (dict(n=1 << 24, ho=128, wo=256), -1, "problem too large for one launch"),
    (dict(inp=None), -1, "null pointer"),
    (dict(grid=None), -1, "null pointer"),
    (dict(go=None), -1, "null pointer"),
    (dict(n=0, **_GS_NONE), 0, None),
    (dict(gi=None, gg=None), 0, None),
    (dict(c=-1, inp=None), -1, _GS_SHAPE),
    (dict(n=0, c=-1), -1, "bad shape N=0 C=-1 in=16x16 out=16x16 outer_div=1 inner=1"),
    (dict(gi=None, gg=None, inp=None), -1, "null pointer"),
)
GS_DET = GS_ATOMIC[:6] + (
    (dict(nin=3), -1, "Nin=3 input maps, the broadcast (4, 4) of N=4 outputs reads more"),
    (dict(nin=-1, n=0), -1, "Nin=-1 input maps, the broadcast (1, 1) of N=0 outputs reads more"),
    (dict(n=8, nin=1, ho=32767, wo=32767, od=8, inner=1), -1, _GS_OVER % (8, 32767, 32767)),
    (dict(n=1 << 26, nin=1 << 26, c=64, ho=64, wo=64), -1, "problem too large for one launch"),
    (dict(nin=1 << 20, c=64, hi=1024, wi=1024), -1, "problem too large for one launch"),
    (dict(nb=_GS_NEED - 1), -1, f"workspace of {_GS_NEED - 1} bytes given, {_GS_NEED} needed"),
    (dict(ws=None), -1, f"workspace of 0 bytes given, {_GS_NEED} needed"),
    (dict(gi=None, gg=None), 0, None),
    (dict(gi=None, gg=None, ws=None, nb=0), 0, None),
    # zero sizes: no output maps still overwrites the Nin input maps' gradient (needs the workspace); none of either
    # and nothing asked for is a return
    (dict(n=0, nin=0, ws=None, nb=0, **_GS_NONE), 0, None),
    (dict(n=0, ws=None, nb=0), -1, f"workspace of 0 bytes given, {_GS_NEED} needed"),
    (dict(n=0, nb=16), -1, f"workspace of 16 bytes given, {_GS_NEED} needed"),
    # two faults
    (dict(c=-1, inp=None), -1, _GS_SHAPE),
    (dict(c=-1, nb=0), -1, _GS_SHAPE),
    (dict(nb=_GS_NEED - 1, inp=None), -1, f"workspace of {_GS_NEED - 1} bytes given, {_GS_NEED} needed"),
    (dict(gi=None, gg=None, inp=None), -1, "null pointer"),
    (dict(gi=None, nb=0, inp=None), -1, "null pointer"),
    (dict(n=0, nin=0, ho=1 << 20, wo=1 << 20), -1, _GS_OVER % (0, 1 << 20, 1 << 20)),
    (dict(n=0, nin=0, ho=1 << 20, wo=1 << 20, ws=None, **_GS_NONE), 0, None),
    (dict(n=8, nin=1, ho=32767, wo=32767, od=8, inner=1, ws=None), -1, _GS_OVER % (8, 32767, 32767)),
    (dict(n=8, nin=1, ho=32767, wo=32767, od=8, inner=1, gi=None, inp=None), -1, "null pointer"),
)
GS_EX = (
    (dict(slots=(2, 1, 0)), -1, _GS_SLOTS),
    (dict(slots=(2, 4, 3)), -1, "bad gradient slots (group 2, stride 4, offset 3)"),
    (dict(slots=(2, 1, 0), c=-1), -1, _GS_SLOTS),
    (dict(slots=(2, 1, 0), inp=None), -1, _GS_SLOTS),
    (dict(slots=(2, 1, 0), n=0), -1, _GS_SLOTS),
)

_OCC_SHAPE = "bad shape M=8 L=40 HW=4096 occ_div=1 (need 1<=L<=32)"
_OCC_NEED = r256(8 * 4 * 81 * 4)
OCC_ATOMIC = (
    (dict(l=40), -1, _OCC_SHAPE),
    (dict(hw=-1), -1, "bad shape M=8 L=9 HW=-1 occ_div=1 (need 1<=L<=32)"),
    (dict(div=0), -1, "bad shape M=8 L=9 HW=4096 occ_div=0 (need 1<=L<=32)"),
    (dict(m=1 << 30, hw=512), -1, "problem too large for one launch"),
    (dict(alpha=None), -1, "null pointer"),
    (dict(occ=None), -1, "null pointer"),
    (dict(go=None), -1, "null pointer"),
    (dict(ga=None), -1, "null pointer"),
    (dict(m=0, alpha=None, occ=None, go=None, ga=None, gocc=None, ws=None, nb=0), 0, None),
    (dict(l=40, ga=None), -1, _OCC_SHAPE),
    (dict(m=0, l=40), -1, "bad shape M=0 L=40 HW=4096 occ_div=1 (need 1<=L<=32)"),
)
OCC_DET = OCC_ATOMIC + (
    (dict(nb=_OCC_NEED - 1), -1, f"workspace of {_OCC_NEED - 1} bytes given, {_OCC_NEED} needed"),
    (dict(ws=None), -1, f"workspace of 0 bytes given, {_OCC_NEED} needed"),
    (dict(gocc=None, ws=None, nb=0, ga=None), -1, "null pointer"),  # no grad_occ: no slab
    (dict(l=40, nb=0), -1, _OCC_SHAPE),
    (dict(nb=_OCC_NEED - 1, ga=None), -1, f"workspace of {_OCC_NEED - 1} bytes given, {_OCC_NEED} needed"),
    (dict(m=0, nb=0), 0, None),  # (an empty slab)
)

_TPS_SHAPE = "bad shape B=8 HW=-4 K3=19"
_TPS_NEED = r256(8 * 1 * 19 * 2 * 4)
TPS_ATOMIC = (
    (dict(hw=-4), -1, _TPS_SHAPE),
    (dict(k3=2), -1, "bad shape B=8 HW=4096 K3=2"),
    (dict(b=4 * 65535 + 1), -1, "bad shape B=262141 HW=4096 K3=19"),
    (dict(basis=None), -1, "null pointer"),
    (dict(gg=None), -1, "null pointer"),
    (dict(gm=None), -1, "null pointer"),
    (dict(b=0, basis=None, gg=None, gm=None, ws=None, nb=0), 0, None),
    (dict(hw=-4, gm=None), -1, _TPS_SHAPE),
    (dict(b=0, hw=-4), -1, "bad shape B=0 HW=-4 K3=19"),
)
_TPS_K3 = "K3=137: the deterministic sum needs the workgroup's table of partials (K3 <= 136)"
TPS_DET = TPS_ATOMIC + (
    (dict(k3=137), -1, _TPS_K3),
    (dict(nb=_TPS_NEED - 1), -1, f"workspace of {_TPS_NEED - 1} bytes given, {_TPS_NEED} needed"),
    (dict(ws=None), -1, f"workspace of 0 bytes given, {_TPS_NEED} needed"),
    (dict(hw=-4, nb=0), -1, _TPS_SHAPE),
    (dict(k3=137, b=0), -1, _TPS_K3),
    (dict(k3=137, nb=0, gm=None), -1, _TPS_K3),
    (dict(nb=_TPS_NEED - 1, gm=None), -1, f"workspace of {_TPS_NEED - 1} bytes given, {_TPS_NEED} needed"),
    (dict(b=0, nb=0), 0, None),
)

_AL_NONE = dict(alpha_lr=None, inp=None, dist=None, occ=None, g_a01=None, g_out=None, g_lr=None, g_dist=None, g_occ=None)
_AL_SHAPE = "bad shape N=6 L=9 H=-16 W=32 scale=4"
_AL_WINDOW = "bad frame window Tw=3 of T=2 or class channels"
_AL_CLS = "bad frame window Tw=3 of T=4 or class channels"
ALPHA_BOTH = (
    (dict(h=-16), -1, _AL_SHAPE),
    (dict(l=33), -1, "bad shape N=6 L=33 H=16 W=32 scale=4"),
    (dict(s=65), -1, "bad shape N=6 L=9 H=16 W=32 scale=65"),
    (dict(t=2), -1, _AL_WINDOW),
    (dict(nl=0), -1, _AL_CLS),
    (dict(nl=33), -1, _AL_CLS),
    (dict(off=4), -1, _AL_CLS),
    (dict(b=-1), -1, "bad shape N=-3 L=9 H=16 W=32 scale=4"),
    (dict(b=0, ws=None, nb=0, **_AL_NONE), 0, None),
    (dict(h=-16, g_lr=None), -1, _AL_SHAPE),
    (dict(t=2, g_lr=None), -1, _AL_WINDOW),
    (dict(b=0, t=2), -1, _AL_WINDOW),
    (dict(b=0, h=-16), -1, "bad shape N=0 L=9 H=-16 W=32 scale=4"),
)
_AL_NULL = "null pointer (one of grad_a01 / grad_alpha_out; scale > 1 needs the (B*Tw, L, Hd, Wd) workspace)"
ALPHA_ATOMIC = ALPHA_BOTH + tuple((dict(kw), -1, _AL_NULL) for kw in (
    dict(alpha_lr=None), dict(occ=None), dict(g_a01=None, g_out=None), dict(g_lr=None), dict(inp=None), dict(ws=None),
    dict(nl=0, dist=None, inp=None, g_lr=None)))
_AL_NEED = _alpha_ws(2, 3, 9, 20, 16, 32, 4)
_AL_NEED0 = _alpha_ws(2, 3, 9, 0, 16, 32, 4)  # without dist: no class slab
ALPHA_DET = ALPHA_BOTH + tuple((dict(kw), -1, "null pointer (one of grad_a01 / grad_alpha_out)") for kw in (
    dict(alpha_lr=None), dict(occ=None), dict(g_a01=None, g_out=None), dict(g_lr=None), dict(inp=None),
    dict(dist=None, inp=None, nb=_AL_NEED0, g_lr=None))) + (
    (dict(nb=_AL_NEED - 1), -1, f"workspace of {_AL_NEED - 1} bytes given, {_AL_NEED} needed"),
    (dict(ws=None), -1, f"workspace of 0 bytes given, {_AL_NEED} needed"),
    (dict(dist=None, nb=_AL_NEED0 - 1), -1, f"workspace of {_AL_NEED0 - 1} bytes given, {_AL_NEED0} needed"),
    (dict(nb=_AL_NEED - 1, g_lr=None), -1, f"workspace of {_AL_NEED - 1} bytes given, {_AL_NEED} needed"),
    (dict(t=2, nb=0), -1, _AL_WINDOW),
    (dict(b=0, nb=0), 0, None),  # (returns before the workspace is looked at)
)

_WP_NONE = dict(flow_lr=None, isobj=None, a01=None, ctx_ts=None, pred_ts=None, occ=None, g_flow=None, g_ctx=None,
                g_dis=None, g_lr=None, g_a01=None, g_occ=None)
_WP_SHAPE = "bad shape N=12 L=40 H=16 W=32 scale=4"
_WP_COUNTS = "bad frame counts T=4 Tw=5 Tc=2 Tp=3"
WARP_BOTH = (
    (dict(l=40), -1, _WP_SHAPE),
    (dict(w=0), -1, "bad shape N=12 L=9 H=16 W=0 scale=4"),
    (dict(tw=5), -1, _WP_COUNTS),
    (dict(tw=0), -1, "bad frame counts T=4 Tw=0 Tc=2 Tp=3"),
    (dict(tc=-1, tp=-3), -1, "bad frame counts T=4 Tw=3 Tc=-1 Tp=-3"),
    (dict(b=0, ws=None, nb=0, **_WP_NONE), 0, None),
    (dict(l=40, g_lr=None), -1, _WP_SHAPE),
    (dict(tw=5, g_lr=None), -1, _WP_COUNTS),
    (dict(b=0, tw=5), -1, _WP_COUNTS),
    (dict(b=0, l=40), -1, "bad shape N=0 L=40 H=16 W=32 scale=4"),
)
_WP_NULL = "null pointer (scale > 1 needs the (M, L, 2, Hd, Wd) workspace)"
WARP_ATOMIC = WARP_BOTH + tuple((dict(kw), -1, _WP_NULL) for kw in (
    dict(flow_lr=None), dict(a01=None), dict(ctx_ts=None), dict(pred_ts=None), dict(occ=None), dict(g_lr=None),
    dict(ws=None))) + (
    (dict(tc=0, ws=None, **_WP_NONE), 0, None),  # no units
)
_WP_NEED = _warp_ws(2, 3, 2, 3, 9, 16, 32, 4)
_WP_NEED_TC0 = _warp_ws(2, 3, 0, 3, 9, 16, 32, 4)
_WP_OVER = ("a texel of grad_a01 may receive more than 2^32 contributions (Tc=3 Tp=3 Hd*Wd=1073676289): no deterministic "
            "sum for this shape")
_WP_OVER_SHAPE = dict(b=1, tc=3, tp=3, l=2, h=32767, w=32767, s=1)
WARP_DET = WARP_BOTH + tuple((dict(kw), -1, "null pointer") for kw in (
    dict(flow_lr=None), dict(a01=None), dict(ctx_ts=None), dict(pred_ts=None), dict(occ=None), dict(g_lr=None),
    dict(tc=0, a01=None), dict(tc=0, occ=None))) + (
    (dict(nb=_WP_NEED - 1), -1, f"workspace of {_WP_NEED - 1} bytes given, {_WP_NEED} needed"),
    (dict(ws=None), -1, f"workspace of 0 bytes given, {_WP_NEED} needed"),
    (_WP_OVER_SHAPE, -1, _WP_OVER),
    (dict(b=1024, t=1024, tw=1024, tc=1, tp=1, l=32, h=1024, w=1024, s=1), -1, "problem too large for one launch"),
    (dict(b=1, tc=1024, tp=511, l=32, h=1024, w=1024, s=1, g_a01=None), -1, "problem too large for one launch"),
    # zero sizes: an empty batch returns before the workspace is looked at; no units (Tc == 0) still overwrites grad_a01
    # and grad_occ, from the workspace
    (dict(b=0, nb=0), 0, None),
    (dict(tc=0, ws=None), -1, f"workspace of 0 bytes given, {_WP_NEED_TC0} needed"),
    (dict(tc=0, nb=_WP_NEED_TC0 - 1), -1, f"workspace of {_WP_NEED_TC0 - 1} bytes given, {_WP_NEED_TC0} needed"),
    # two faults
    (dict(tw=5, nb=0), -1, _WP_COUNTS),
    (dict(nb=_WP_NEED - 1, g_lr=None), -1, f"workspace of {_WP_NEED - 1} bytes given, {_WP_NEED} needed"),
    (dict(_WP_OVER_SHAPE, b=0), -1, _WP_OVER),
    (dict(_WP_OVER_SHAPE, ws=None, a01=None), -1, _WP_OVER),
    (dict(_WP_OVER_SHAPE, g_a01=None, ws=None), -1,
     f"workspace of 0 bytes given, {_warp_ws(1, 3, 3, 3, 2, 32767, 32767, 1)} needed"),
    (dict(_WP_OVER_SHAPE, g_a01=None, b=0, ws=None), 0, None),
)

PINNED = {
    "waldo_grid_sample2d_bwd": (_gs_args, GS_ATOMIC),
    "waldo_grid_sample2d_ex_bwd": (_gs_args, GS_ATOMIC + GS_EX),
    "waldo_grid_sample2d_bwd_det": (_gs_args, GS_DET),
    "waldo_grid_sample2d_ex_bwd_det": (_gs_args, GS_DET + GS_EX),
    "waldo_occ_composite_bwd": (_occ_args, OCC_ATOMIC),
    "waldo_occ_composite_bwd_det": (_occ_args, OCC_DET),
    "waldo_tps_grid_bwd": (_tps_args, TPS_ATOMIC),
    "waldo_tps_grid_bwd_det": (_tps_args, TPS_DET),
    "waldo_flow_ctx_alpha_bwd": (_alpha_args, ALPHA_ATOMIC),
    "waldo_flow_ctx_alpha_bwd_det": (_alpha_args, ALPHA_DET),
    "waldo_flow_ctx_warp_bwd": (_warp_args, WARP_ATOMIC),
    "waldo_flow_ctx_warp_bwd_det": (_warp_args, WARP_DET),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_refusals_and_early_returns_are_pinned(lib, name):
    build_args, rows = PINNED[name]
    fn = getattr(lib, name)
    for kw, rc, tail in rows:
        lib.waldo_set_debug_option(-1, 0)  # (a refusal of its own: the message buffer now holds something else)
        got = fn(*build_args(name, **kw))
        msg = _msg(lib)
        print(name, kw, got, msg)
        assert got == rc, (name, kw, msg)
        if rc != 0:
            assert msg == f"{name}: {tail}", (name, kw)
        else:  # nothing launched, nothing reported
            assert msg == "waldo_set_debug_option: unknown option -1", (name, kw)


def test_warp_composite_bwd_workspace_refusals_are_pinned(lib):
    """The default backward of the fused warp / composite shares the workspace refusal with the deterministic ones: its
    checks, with their order, for fp32 layers (a workspace is optional, a short one refused) and 16-bit layers (required)."""
    need = lib.waldo_warp_composite_bwd_workspace_bytes(2, 8, 64, 96, 19)
    assert need > 0
    note = " (a 16-bit layer stack has no generic backward)"
    unserved = ("a 16-bit layer stack needs the two-kernel backward (K3 == 19, L <= 17, W % 4 == 0, H, W >= 2, "
                "WALDO_DEBUG_BWD_GENERIC off); not served: L=8 H=64 W=96 K3=15 -- pass fp32 layers")

    def call(name, code=None, gl=FAKE, ws=FAKE, nb=BIG, F=2, L=8, K3=19):
        tail = [] if code is None else [code]
        return getattr(lib, name)(FAKE, FAKE, FAKE, FAKE, FAKE, None, gl, FAKE, FAKE, ws, nb, F, L, 64, 96, K3, 0.0, *tail, None)

    rows = (
        ("waldo_warp_composite_bwd", dict(nb=need - 1), -1, f"workspace of {need - 1} bytes given, {need} needed"),
        ("waldo_warp_composite_bwd", dict(nb=need - 1, gl=None), -1, "null pointer"),
        ("waldo_warp_composite_bwd", dict(gl=None, ws=None), -1, "null pointer"),
        ("waldo_warp_composite_bwd", dict(L=99, nb=0), -1,
         "unsupported shape F=2 L=99 H=64 W=96 K3=19 (need 1<=L<=32, 3<=K3<=32)"),
        ("waldo_warp_composite_bwd", dict(F=0, ws=None, nb=0, gl=None), 0, None),
        ("waldo_warp_composite_bwd_dt", dict(code=0, nb=need - 1), -1, f"workspace of {need - 1} bytes given, {need} needed"),
        ("waldo_warp_composite_bwd_dt", dict(code=7), -1, "unknown dtype 7 for layers (WALDO_DTYPE_F32 / _F16 / _BF16)"),
    ) + tuple(row for code in (1, 2) for row in (
        ("waldo_warp_composite_bwd_dt", dict(code=code, ws=None, nb=BIG), -1, f"workspace of 0 bytes given, {need} needed" + note),
        ("waldo_warp_composite_bwd_dt", dict(code=code, nb=need - 1), -1, f"workspace of {need - 1} bytes given, {need} needed" + note),
        ("waldo_warp_composite_bwd_dt", dict(code=code, nb=0, gl=None), -1, "null pointer"),
        ("waldo_warp_composite_bwd_dt", dict(code=code, K3=15, ws=None), -1, unserved),
        ("waldo_warp_composite_bwd_dt", dict(code=code, K3=15, F=0), -1, unserved),
        ("waldo_warp_composite_bwd_dt", dict(code=code, F=0, ws=None, nb=0, gl=None), 0, None),
    ))
    for name, kw, rc, tail in rows:
        lib.waldo_set_debug_option(-1, 0)  # (a refusal of its own: the message buffer now holds something else)
        got = call(name, **kw)
        msg = _msg(lib)
        assert got == rc, (name, kw, msg)
        assert msg == (f"{name}: {tail}" if rc else "waldo_set_debug_option: unknown option -1"), (name, kw)


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
