"""CPU: the restatement of the supervision targets (tests/supervision_ref.py) against the fixture recorded from the
reference's own EdgeExtractor (tests/golden/flow_edges_reference.npz, tools_dev/make_supervision_golden.py) and, where the
reference tree is present, against the class itself; the blur's definition; and the C ABI and the Python surface of
include/waldo_hip.h "Supervision targets" as far as they go without a GPU: argument validation on the host -- no kernel
is launched."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import supervision_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "flow_edges_reference.npz")
REF_ROOT = os.environ.get("WALDO_REFERENCE_ROOT", "/root/reference")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def real_flow():
    from waldo_amd.tools.io import read_flo
    return read_flo(os.path.join(ROOT, "tests", "golden", "demo_flow.flo"))[None]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# ---------------------------------------------------------------------------------------------------------------------
def _same(edge, dominant, want_edge, want_dominant, what):
    err = (edge - torch.from_numpy(want_edge)).abs().max().item()
    flips = int((dominant.numpy() != want_dominant.astype(np.float32)).sum())
    print(f"[supervision] {what}: |edge - reference| {err:.3e}, dominant flips {flips}")
    assert err <= 1e-6 and flips == 0, (what, err, flips)


@pytest.mark.parametrize("k", [3, 7, 15])
def test_restated_flow_edges_equal_the_fixture(golden, k):
    edge, dominant = R.flow_edges(torch.from_numpy(golden["flow"]), k)
    assert edge.shape == dominant.shape == (2, 3, 1, 24, 40)
    _same(edge, dominant, golden[f"edge_k{k}"], golden[f"dominant_k{k}"], f"k={k}")


def test_restated_flow_edges_equal_the_fixture_on_the_real_flow(golden):
    flow = real_flow()
    assert flow.shape == (1, 2, 128, 256)
    edge, dominant = R.flow_edges(flow, 15)
    _same(edge, dominant, golden["real_edge_k15"], golden["real_dominant_k15"], "real flow, k=15")
    # both sides of the recipe's threshold are populated: the fixture can tell a wrong threshold
    assert 0.1 < float((edge > 0.02).float().mean()) < 0.9


@pytest.mark.live_ref
def test_restated_flow_edges_equal_the_reference_live(golden):
    if not os.path.exists(os.path.join(REF_ROOT, "models", "modules", "edge.py")):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("_make_supervision_golden",
                                                  os.path.join(ROOT, "tools_dev", "make_supervision_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    Edge = maker.load_edge_extractor(REF_ROOT)
    g = torch.Generator().manual_seed(5)
    flow = 0.05 * torch.randn(2, 2, 2, 17, 33, generator=g)
    with torch.no_grad():
        for k in (3, 5, 15):
            want_edge, want_dominant = Edge(k)(flow)
            edge, dominant = R.flow_edges(flow, k)
            _same(edge, dominant, want_edge.numpy(), want_dominant.numpy(), f"live k={k}")


@pytest.mark.parametrize("k,sigma", [(3, 2.0), (23, 2.0), (23, 3.0), (31, 0.7)])
def test_blur_weights_equal_the_closed_form(k, sigma):
    w = R.gaussian_weights(k, sigma, torch.float64)
    t = np.arange(k, dtype=np.float64) - (k - 1) / 2
    want = np.exp(-0.5 * (t / sigma) ** 2)
    want /= want.sum()
    assert np.allclose(w.numpy(), want, rtol=0, atol=1e-15)
    assert abs(float(w.sum()) - 1.0) < 1e-15 and torch.equal(w, w.flip(0))
    w32 = R.gaussian_weights(k, sigma, torch.float32)
    assert np.allclose(w32.numpy(), want, rtol=0, atol=2e-7)


@pytest.mark.parametrize("k", [3, 23])
def test_blur_keeps_a_constant_image_constant(k):
    x = torch.full((2, 3, 24, 40), 0.37, dtype=torch.float64)
    assert (R.gaussian_blur(x, 2.0, k) - 0.37).abs().max().item() < 1e-15
    x32 = torch.full((1, 2, 12, 30), -1.25)
    assert (R.gaussian_blur(x32, 2.0, k) + 1.25).abs().max().item() < 1e-6


def test_blur_reflects_without_repeating_the_border():
    x = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
    x[0, 0, 0, 1] = 1.0  # one step inside the border: reflection sees it twice from row 0's window, replication would not
    w = R.gaussian_weights(3, 2.0, torch.float64)
    y = R.gaussian_blur(x, 2.0, 3)
    assert abs(y[0, 0, 0, 0].item() - float(w[1] * (w[0] + w[2]))) < 1e-15
    assert abs(y[0, 0, 1, 1].item() - float(w[0] * w[1])) < 1e-15
    x[0, 0, 0, 1], x[0, 0, 1, 0] = 0.0, 1.0
    assert abs(R.gaussian_blur(x, 2.0, 3)[0, 0, 0, 0].item() - float((w[0] + w[2]) * w[1])) < 1e-15


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a GPU (the pointers are never dereferenced: every case is refused, or returns, before a launch)
# ---------------------------------------------------------------------------------------------------------------------
P = 64  # a non-null "pointer"


def edges(lib, flow=P, edge=P, dom=P, n=1, c=2, h=24, w=40, k=15, eps=1e-6):
    return lib.waldo_flow_edges_fwd(flow, edge, dom, n, c, h, w, k, eps, None)


def blur(lib, x=P, y=P, p=3, h=24, w=40, k=23, sigma=2.0):
    return lib.waldo_gaussian_blur_fwd(x, y, p, h, w, k, sigma, None)


def props(lib, ptrs=(P,) * 6, fg=1, bg=2, other=4, n=1, nl=20, hw=960):
    return lib.waldo_mov_props_fwd(ptrs[0], ptrs[1], fg, bg, other, *ptrs[2:], n, nl, hw, None)


def finish(lib, ptrs=(P,) * 11, flags=1, n=1, hw=960, thresh=0.02):
    return lib.waldo_mov_finish_fwd(*ptrs[:7], thresh, 0.005, 0.25, 0.0, flags, *ptrs[7:], n, hw, None)


def cell_fwd(lib, ptrs=(P,) * 8, ws=1 << 20, f=2, no=16, h=24, w=40, k=9.0, eps=0.0):
    return lib.waldo_cell_distance_fwd(*ptrs, ws, f, no, h, w, k, eps, None)


def cell_bwd(lib, ptrs=(P,) * 10, ws=1 << 20, f=2, no=16, h=24, w=40, k=9.0, eps=0.0):
    return lib.waldo_cell_distance_bwd(*ptrs, ws, f, no, h, w, k, eps, None)


def test_symbols_are_exported_bound_and_described(lib):
    from waldo_amd import _lib
    names = ("waldo_flow_edges_fwd", "waldo_gaussian_blur_fwd", "waldo_mov_props_fwd", "waldo_mov_finish_fwd",
             "waldo_cell_distance_fwd", "waldo_cell_distance_bwd")
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "waldo_cell_distance_workspace_bytes" in _lib.PLAIN
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Supervision targets:"):]
    for needle in names + ("NO FLOAT ATOMICS", "ties go to the lowest index", "Reflection padding"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


@pytest.mark.parametrize("call,kw,msg", [
    (edges, dict(k=4), b"kernel size"), (edges, dict(k=14), b"kernel size"), (edges, dict(k=17), b"kernel size"),
    (edges, dict(k=1), b"kernel size"), (edges, dict(k=15, h=7), b"bad shape"), (edges, dict(k=15, w=7), b"bad shape"),
    (edges, dict(k=3, h=1), b"bad shape"), (edges, dict(c=3), b"bad arguments"), (edges, dict(c=0), b"bad arguments"),
    (edges, dict(n=-1), b"bad arguments"), (edges, dict(eps=-1.0), b"bad arguments"),
    (edges, dict(flow=None), b"null pointer"), (edges, dict(edge=None), b"null pointer"),
    (edges, dict(dom=None), b"null pointer"),
    (blur, dict(k=22), b"kernel size"), (blur, dict(k=33), b"kernel size"), (blur, dict(k=23, h=11), b"bad shape"),
    (blur, dict(k=23, w=11), b"bad shape"), (blur, dict(sigma=0.0), b"sigma"), (blur, dict(sigma=float("nan")), b"sigma"),
    (blur, dict(p=-1), b"bad arguments"), (blur, dict(x=None), b"null pointer"), (blur, dict(y=None), b"null pointer"),
    (props, dict(nl=33), b"Nl=33"), (props, dict(nl=0), b"Nl=0"), (props, dict(nl=3, other=8), b"at or above"),
    (props, dict(n=-1), b"bad shape"), (props, dict(hw=0), b"bad shape"),
    (props, dict(ptrs=(None,) + (P,) * 5), b"null pointer"), (props, dict(ptrs=(P,) * 5 + (None,)), b"null pointer"),
    (finish, dict(flags=32), b"bad flags"), (finish, dict(flags=8 | 16), b"bad flags"),
    (finish, dict(thresh=float("inf")), b"not finite"), (finish, dict(n=-1), b"bad shape"),
    (finish, dict(ptrs=(P,) * 10 + (None,)), b"null pointer"), (finish, dict(ptrs=(None,) + (P,) * 10), b"null pointer"),
    (cell_fwd, dict(no=32), b"No=32"), (cell_fwd, dict(no=0), b"No=0"), (cell_fwd, dict(f=-1), b"bad shape"),
    (cell_fwd, dict(h=0), b"bad shape"), (cell_fwd, dict(k=0.0), b"bad K"), (cell_fwd, dict(eps=float("nan")), b"bad K"),
    (cell_fwd, dict(ws=16), b"workspace"), (cell_fwd, dict(ptrs=(None,) + (P,) * 7), b"null pointer"),
    (cell_fwd, dict(ptrs=(P,) * 5 + (None, P, P)), b"null pointer"),          # out
    (cell_fwd, dict(ptrs=(P,) * 7 + (None,)), b"null pointer"),                # workspace
    (cell_bwd, dict(no=32), b"No=32"), (cell_bwd, dict(ws=16), b"workspace"),
    (cell_bwd, dict(ptrs=(P,) * 5 + (None,) + (P,) * 4), b"null pointer"),     # chosen
    (cell_bwd, dict(ptrs=(P, P, None) + (P,) * 7), b"null pointer"),           # grad_fg without fg_mask
])
def test_entry_points_reject_bad_arguments_before_any_launch(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.waldo_last_error_string(), (call.__name__, kw, lib.waldo_last_error_string())


def test_fg_mask_is_optional_but_validated_last(lib):
    """The centre term passes no fg_mask: with F == 0 the call returns before anything is read."""
    assert cell_fwd(lib, ptrs=(None,) * 8, f=0, ws=0) == 0
    assert cell_bwd(lib, ptrs=(None,) * 10, f=0, ws=0) == 0


def test_empty_batches_return_ok_without_a_launch(lib):
    assert edges(lib, flow=None, edge=None, dom=None, n=0) == 0
    assert blur(lib, x=None, y=None, p=0) == 0
    assert props(lib, ptrs=(None,) * 6, n=0) == 0
    assert finish(lib, ptrs=(None,) * 11, n=0) == 0


def test_workspace_query(lib):
    q = lib.waldo_cell_distance_workspace_bytes
    assert q(28, 16, 128 * 256) == 28 * 16 * 16 * 3 * 4  # 16 chunks of 2048 pixels per frame
    assert q(6, 5, 17 * 33) == 512 and q(6, 5, 17 * 33) % 256 == 0
    assert q(1, 32, 64) == 0 and q(1, 0, 64) == 0 and q(-1, 4, 64) == 0


# ---------------------------------------------------------------------------------------------------------------------
# Python-side errors
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_inputs():
    g = torch.Generator().manual_seed(0)
    flow = 0.05 * torch.randn(1, 2, 2, 24, 40, generator=g)
    lyt = torch.randn(1, 2, 20, 24, 40, generator=g)
    pose = torch.randn(1, 2, 5, 16, 2, generator=g)
    mask = torch.rand(1, 2, 1, 24, 40, generator=g)
    return flow, lyt, pose, mask


TARGET = dict(flow_thresh=0.02, mov_obj_thresh=0.005, blur_sigma=2.0, edge_size=15)


def test_wrappers_have_no_cpu_fallback():
    from waldo_amd import supervision as S
    from waldo_amd._lib import WaldoHipError
    flow, lyt, pose, mask = _cpu_inputs()
    with pytest.raises(WaldoHipError):
        S.flow_edges(flow)
    with pytest.raises(WaldoHipError):
        S.gaussian_blur(lyt, 2.0)
    with pytest.raises(WaldoHipError):
        S.moving_object_target(flow, lyt, [0], [1], [2], **TARGET)
    with pytest.raises(WaldoHipError):
        S.cell_distance(pose, (4, 4), mask, mask)
    with pytest.raises(WaldoHipError):
        S.cell_distance(pose, (4, 4), mask, mask, center=True)
    target = S.MovingObjectTarget(mask, mask, mask, flow, mask, mask)
    with pytest.raises(WaldoHipError):
        S.recipe_terms(torch.zeros(1, 2, 6, 24, 40), flow[:, 1:], flow, lyt, pose, (4, 4), target)


def test_wrappers_refuse_bad_arguments():
    import waldo_amd
    from waldo_amd import supervision as S
    assert waldo_amd.supervision is S
    flow, lyt, pose, mask = _cpu_inputs()
    with pytest.raises(ValueError, match="2 channels"):
        S.flow_edges(lyt)
    with pytest.raises(ValueError, match="float32"):
        S.flow_edges(flow.double())
    with pytest.raises(ValueError, match="requires grad"):
        S.flow_edges(flow.clone().requires_grad_())
    with pytest.raises(ValueError, match="requires grad"):
        S.moving_object_target(flow, lyt.clone().requires_grad_(), [0], [1], [2], **TARGET)
    with pytest.raises(ValueError, match="requires grad"):
        S.moving_object_target(flow.clone().requires_grad_(), lyt, [0], [1], [2], **TARGET)
    with pytest.raises(ValueError, match="channel 20"):
        S.moving_object_target(flow, lyt, [20], [1], [2], **TARGET)
    with pytest.raises(ValueError, match="disagree"):
        S.moving_object_target(flow[:, :1], lyt, [0], [1], [2], **TARGET)
    with pytest.raises(ValueError, match="33 layout channels"):
        S.moving_object_target(flow, torch.zeros(1, 2, 33, 24, 40), [0], [1], [2], **TARGET)
    with pytest.raises(ValueError, match="use_flow_nobg"):
        S.moving_object_target(flow, lyt, [0], [1], [2], use_flow_nobg=True, use_dominant_flow_other=True, **TARGET)
    with pytest.raises(ValueError, match="no cell"):
        S.cell_distance(pose, (1, 16), mask, mask)
    with pytest.raises(ValueError, match="obj_pose"):
        S.cell_distance(pose, (3, 4), mask, mask)
    with pytest.raises(ValueError, match="No = 32"):
        S.cell_distance(torch.zeros(1, 2, 32, 16, 2), (4, 4), mask, mask)
    with pytest.raises(ValueError, match="fg_mask"):
        S.cell_distance(pose, (4, 4), mask, mask[:, :1])
    with pytest.raises(ValueError, match="requires grad"):
        S.cell_distance(pose, (4, 4), mask.clone().requires_grad_(), mask)


def test_cell_moments_give_the_references_distances():
    """The analytic form the kernel evaluates -- K |g|^2 - 2 g . S1 + S2 from ``cell_moments`` -- against the reference's
    expanded tensor (synthesizer.py:970-974), in float64."""
    from waldo_amd import supervision as S
    from waldo_amd.tools.utils import get_grid
    g = torch.Generator().manual_seed(3)
    pose = torch.randn(2, 3, 4, 6, 2, generator=g, dtype=torch.float64)
    cell, centre = S.cell_moments(pose, (2, 3))
    assert cell.shape == centre.shape == (2, 3, 4, 3)
    grid = get_grid(5, 7).double().view(-1, 2)
    ones = torch.ones(2, 3, 1, 5, 7, dtype=torch.float64)
    for mom, k, pick in ((cell, 2, 0), (centre, 1, 1)):
        dis = k * (grid ** 2).sum(-1) - 2 * mom[..., :2] @ grid.t() + mom[..., 2:]          # (2, 3, 4, 35)
        want = R.cell_distance(pose, (2, 3), ones, torch.zeros_like(ones))[pick]
        assert abs(dis.min(dim=2)[0].mean().item() - want.item()) < 1e-12


def test_lvd_step_refuses_an_unknown_objective():
    from waldo_amd.tools.lvd_step import LvdStep, RECIPE_TARGET, RECIPE_WEIGHTS
    with pytest.raises(ValueError, match="objective"):
        LvdStep(1, torch.device("cpu"), objective="recipes")
    assert RECIPE_WEIGHTS == {"cell_dis": 10.0, "l1_flow": 1000.0, "reg_mov": 10.0, "ent_flt_edge": 1.0}
    assert RECIPE_TARGET["edge_size"] == 15 and RECIPE_TARGET["other_idx"] == [9]
