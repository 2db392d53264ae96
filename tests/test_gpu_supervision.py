"""GPU: waldo_amd.supervision against its restatement in framework ops (tests/supervision_ref.py) in fp32 and fp64, and
against the fixture recorded from the reference's EdgeExtractor (tests/golden/flow_edges_reference.npz).

Continuous outputs go through tests/parity.py::close.  A 0 / 1 map is a threshold decision: a pixel may differ from the
fp32 restatement only where the fp64 restatement's DECIDING quantity (flow_edge - flow_thresh, delta_flow -
mov_obj_thresh, sum flow^2 - sum mean^2) lies within a margin of zero; the margin is 16 x the largest |fp32 - fp64| of that
quantity, measured here and printed, and at most 0.5 % of the pixels may be excused that way (``decisions``).

The ``check_*`` helpers take the candidate as a callable: the GPU tests hand them the kernels' wrappers,
tests/test_supervision_sensitivity_cpu.py the faulted restatements of tests/supervision_tiled.py.  The cases beyond one
chunk, one tile row and the limits (31 objects, 31 taps, 32 channels) come from tests/supervision_regimes.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import supervision_ref as R  # noqa: E402
import supervision_regimes as SR  # noqa: E402
from parity import TOL, close  # noqa: E402
from supervision_regimes import BG, FG, NL, OTHER, THRESH, target_inputs  # noqa: E402, F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_X, EXCUSED = 16.0, 0.005


@pytest.fixture(scope="module")
def S():
    from waldo_amd import supervision
    return supervision


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "flow_edges_reference.npz"))


def decisions(got, ref32, deciding, what, cap=EXCUSED):
    """``got`` (the device's map) equals ``ref32`` except where a deciding quantity is within its margin of zero.
    ``deciding``: pairs (fp32, fp64) of quantity - threshold.  Values that are not decisions (a soft layout's
    other_prop under use_dominant_flow_other) count as different beyond parity.TOL."""
    got, ref32 = got.detach().cpu().double(), ref32.detach().cpu().double()
    near = torch.zeros_like(ref32, dtype=torch.bool)
    for i, (q32, q64) in enumerate(deciding):
        noise = (q32.double() - q64).abs().max().item()
        margin = MARGIN_X * noise
        near_q = q64.abs() <= margin
        print(f"[decisions] {what}: quantity {i}: fp32 noise {noise:.3e}, margin {margin:.3e}, "
              f"{int(near_q.sum())} of {near_q.numel()} pixels within it")
        near |= near_q
    differ = (got - ref32).abs() > TOL
    print(f"[decisions] {what}: {int(differ.sum())} pixels differ, {int((differ & ~near).sum())} of them unexcused")
    assert not (differ & ~near).any(), (what, int((differ & ~near).sum()))
    assert differ.float().mean().item() <= cap, what


# ---------------------------------------------------------------------------------------------------------------------
# flow edges
# ---------------------------------------------------------------------------------------------------------------------
def check_edges(S, dev, flow, k, what, want=None):
    e32, d32, m32 = R.flow_edges_parts(flow, k)
    e64, d64, m64 = R.flow_edges_parts(flow.double(), k)
    edge, dominant = S.flow_edges(flow.to(dev), k)
    assert edge.shape == e32.shape and dominant.shape == d32.shape
    close(edge, e32, what=f"flow_edge {what}", exact=e64)
    if want is not None:
        close(edge, torch.from_numpy(want[0]), what=f"flow_edge {what} vs the reference's", exact=e64)
        assert np.array_equal(d32.numpy(), want[1].astype(np.float32))
    decisions(dominant, d32, [(m32, m64)], f"dominant_flow {what}")
    assert set(dominant.unique().tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("k", [3, 7, 15])
def test_flow_edges_on_the_fixture(S, dev, golden, k):
    """24 x 40: no multiple of the 16 x 64 tile, two tile rows."""
    check_edges(S, dev, torch.from_numpy(golden["flow"]), k, f"k={k}", (golden[f"edge_k{k}"], golden[f"dominant_k{k}"]))


def test_flow_edges_where_the_halo_reflects_across_both_borders(S, dev):
    """8 x 72 at k = 15: pad 7 against height 8 -- one tile's halo reflects at the top AND the bottom; two tile columns."""
    g = torch.Generator().manual_seed(11)
    flow = 0.03 * torch.randn(3, 2, 8, 72, generator=g)
    check_edges(S, dev, flow, 15, "8x72 k=15")
    check_edges(S, dev, flow[:, :, :, :9].contiguous(), 15, "8x9 k=15")


def test_flow_edges_on_the_real_flow(S, dev, golden):
    from waldo_amd.tools.io import read_flo
    flow = read_flo(os.path.join(ROOT, "tests", "golden", "demo_flow.flo"))[None]
    check_edges(S, dev, flow, 15, "real 128x256 k=15", (golden["real_edge_k15"], golden["real_dominant_k15"]))


@pytest.mark.parametrize("h,w,k", SR.EDGE_CASES)
def test_flow_edges_across_tile_rows_and_columns(S, dev, h, w, k):
    """33 x 130: three tile rows and three tile columns, the last of one pixel row and of two pixels; 17 x 65: two and
    two, the last of one row and one pixel."""
    check_edges(S, dev, SR.edge_input(h, w), k, f"{h}x{w} k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian blur
# ---------------------------------------------------------------------------------------------------------------------
OLD_BLUR_CASES = [(k, c, h, w) for h, w in ((24, 40), (12, 70)) for c in (1, 3, 20) for k in (3, 23)]


def old_blur_input(k, c, h, w):
    return torch.randn(2, c, h, w, generator=torch.Generator().manual_seed(100 * k + c))


def device_blur(S, dev):
    return lambda x, sigma, k: S.gaussian_blur(x.to(dev), sigma, k)


def check_blur(blur, x, sigma, k, what, refs=None):
    """``blur(x, sigma, k)`` against the restatement; ``refs``: its (fp32, fp64) results where they are shared."""
    r32, r64 = refs if refs is not None else (R.gaussian_blur(x, sigma, k), R.gaussian_blur(x.double(), sigma, k))
    got = blur(x, sigma, k)
    assert got.shape == x.shape
    close(got, r32, what=what, exact=r64)


@pytest.mark.parametrize("k", [3, 23])
@pytest.mark.parametrize("c", [1, 3, 20])
@pytest.mark.parametrize("h,w", [(24, 40), (12, 70)])
def test_gaussian_blur(S, dev, k, c, h, w):
    """12 x 70: pad 11 against height 12, two tile columns; 24 x 40: no multiple of the 32 x 64 tile."""
    check_blur(device_blur(S, dev), old_blur_input(k, c, h, w), 2.0, k, f"blur k={k} C={c} {h}x{w}")


def test_gaussian_blur_keeps_leading_dimensions_and_a_constant(S, dev):
    x = torch.full((2, 3, 2, 24, 40), 0.37, device=dev)
    got = S.gaussian_blur(x, 3.0)
    assert got.shape == x.shape and (got - 0.37).abs().max().item() < 1e-6


@pytest.mark.parametrize("h,w,k,sigma", SR.BLUR_CASES)
def test_gaussian_blur_across_tile_rows(S, dev, h, w, k, sigma):
    """40 x 72: two tile rows and columns, every halo row of the second tile row a neighbour's; 33 x 65: a tile row of one
    pixel row and a tile column of one pixel; 65 x 40: three tile rows; 16 x 70 at k = 31: pad 15 against height 16.
    k = 31 is the size the two LDS buffers are made for."""
    check_blur(device_blur(S, dev), SR.blur_input(h, w), sigma, k, f"blur k={k} sigma={sigma} {h}x{w}",
               SR.blur_refs(h, w, k, sigma))


# ---------------------------------------------------------------------------------------------------------------------
# moving-object target
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def target_case():
    """The 24 x 40 inputs (supervision_regimes.target_inputs) and the restatement's targets (fp32, fp64) per option set,
    each computed once."""
    flow, lyt, _, _, refs = SR.target_refs()
    return flow, lyt, refs


def check_target_fixture(refs, thresh, what="24x40"):
    """What a target fixture must be for the checks below to mean something: both sides of every threshold populated,
    few pixels within the margin of one, the ``== 0`` branch of the blurred weight taken on frame (0, 1) alone."""
    r = refs()[0]
    for name, frac in (("flow_edge", r["flow_edge"].mean().item()), ("dominant_flow", r["dominant_flow"].mean().item()),
                       ("mov_obj_mask", r["mov_obj_mask"].mean().item()),
                       ("fg_prop > 0", (r["fg_prop"] > 0).float().mean().item()),
                       ("nobg_prop > 0", (r["nobg_prop"] > 0).float().mean().item())):
        print(f"[target fixture {what}] {name}: {frac:.3f} of the pixels")
        assert 0.1 <= frac <= 0.9, (name, frac)
    # the restatement alone stays far inside the cap: few pixels of THIS fixture sit within the margin of a threshold
    r32, r64 = refs()
    for name, t in (("edge_raw", thresh["flow_thresh"]), ("delta_flow", thresh["mov_obj_thresh"]),
                    ("dominant_margin", 0.0)):
        noise = (r32[name].double() - r64[name]).abs().max().item()
        near = ((r64[name] - t).abs() <= MARGIN_X * noise).float().mean().item()
        flips = ((r32[name] > t) != (r64[name] > t)).float().mean().item()
        print(f"[target fixture {what}] {name}: fp32 noise {noise:.3e}, {near:.5f} of the pixels within {MARGIN_X:g} x of "
              f"it, {flips:.5f} decided differently in fp32 and fp64")
        assert near <= EXCUSED / 2 and flips <= EXCUSED / 2, name
    blurred0 = R.gaussian_blur(1 - r["fg_prop"], thresh["blur_sigma"])
    assert (blurred0[0, 1] == 0).all() and (blurred0[0, 0] != 0).any()  # the `== 0` branch runs, and not everywhere


def test_target_fixture_populates_both_sides_of_every_threshold(target_case):
    check_target_fixture(target_case[2], THRESH)


OPTION_SETS = [dict(), dict(use_fg=True), dict(use_nobg=True), dict(use_nobg_edge=True, nobg_edge_mul=0.3),
               dict(use_flow_nobg=True), dict(use_dominant_flow_other=True), dict(reg_bg_mul=0.0),
               dict(use_fg=True, use_dominant_flow_other=True),                                          # the recipe's
               dict(use_fg=True, use_nobg=True, use_nobg_edge=True, nobg_edge_mul=-0.5, use_flow_nobg=True)]


def device_target(S, dev):
    return lambda flow, lyt, *lists, **kw: S.moving_object_target(flow.to(dev), lyt.to(dev), *lists, **kw)


def deciding(r32, r64, thresh):
    """The (fp32, fp64) pairs of quantity - threshold behind flow_edge, delta_flow and dominant_flow."""
    return ((r32["edge_raw"] - thresh["flow_thresh"], r64["edge_raw"] - thresh["flow_thresh"]),
            (r32["delta_flow"] - thresh["mov_obj_thresh"], r64["delta_flow"] - thresh["mov_obj_thresh"]),
            (r32["dominant_margin"], r64["dominant_margin"]))


def check_target(target, flow, lyt, lists, thresh, refs, opts, what=""):
    """``target(flow, lyt, fg, bg, other, **options)`` against the restatement's (fp32, fp64) of ``refs(**opts)``, field
    by field.  Frame (0, 1) of every fixture is all foreground: its mean_bg_flow is exactly 0."""
    r32, r64 = refs(**opts)
    got = target(flow, lyt, *lists, **thresh, **opts)
    what = (what + " " if what else "") + ("+".join(opts) or "plain")
    for name in got._fields:
        assert getattr(got, name).shape == r32[name].shape and not getattr(got, name).requires_grad, name
    close(got.fg_prop, r32["fg_prop"], what=f"fg_prop {what}", exact=r64["fg_prop"])
    close(got.mean_bg_flow, r32["mean_bg_flow"], what=f"mean_bg_flow {what}", exact=r64["mean_bg_flow"])
    assert (got.mean_bg_flow[0, 1] == 0).all()
    edge, delta, dominant = deciding(r32, r64, thresh)
    decisions(got.flow_edge, r32["flow_edge"], [edge], f"flow_edge {what}")
    decisions(got.dominant_flow, r32["dominant_flow"], [dominant], f"dominant_flow {what}")
    decisions(got.mov_obj_mask, r32["mov_obj_mask"], [edge, delta, dominant], f"mov_obj_mask {what}")
    decisions(got.mov_obj, r32["mov_obj"], [edge, delta, dominant], f"mov_obj {what}")
    return got


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "+".join(k for k in o) or "plain")
def test_moving_object_target(S, dev, target_case, opts):
    flow, lyt, refs = target_case
    check_target(device_target(S, dev), flow, lyt, (FG, BG, OTHER), THRESH, refs, opts)


def test_moving_object_target_accepts_frames_without_a_clip_dimension(S, dev, target_case):
    flow, lyt, refs = target_case
    a = S.moving_object_target(flow.to(dev), lyt.to(dev), FG, BG, OTHER, **THRESH, use_fg=True)
    b = S.moving_object_target(flow.view(6, 2, 24, 40).to(dev), lyt.view(6, NL, 24, 40).to(dev), FG, BG, OTHER, **THRESH,
                               use_fg=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(y.shape), y)


@pytest.mark.parametrize("opts", [SR.RECIPE_OPTS, SR.ALL_OPTS], ids=["recipe", "all"])
@pytest.mark.parametrize("h,w,edge_size", SR.TARGET_CASES)
def test_moving_object_target_across_tiles(S, dev, h, w, edge_size, opts):
    """40 x 72 and 37 x 70: two rows and two columns of the blur's tiles (the second row of 8 and of 5 pixel rows), three
    tile rows of the edges', 12 and 11 workgroups of 256 pixels per frame with a ragged last one."""
    flow, lyt, lists, thresh, refs = SR.target_refs(h, w, edge_size)
    check_target(device_target(S, dev), flow, lyt, lists, thresh, refs, opts, f"{h}x{w} e={edge_size}")


def test_moving_object_target_on_32_channels_with_channel_31_listed(S, dev):
    """Nl = 32: the lists name channels 31, 30 and 0 -- bit 31 of the masks, and no shift by Nl in their check."""
    flow, lyt, lists, thresh, refs = SR.target_refs(40, 72, 15, layout="wide")
    assert lyt.shape[2] == 32 and {31, 30, 0} <= set(lists[0] + lists[1]) and (lyt[:, :, 31] > 0).any()
    check_target(device_target(S, dev), flow, lyt, lists, thresh, refs, SR.RECIPE_OPTS, "Nl=32")
    check_target(device_target(S, dev), flow, lyt, lists, thresh, refs, SR.ALL_OPTS, "Nl=32")


def test_moving_object_target_recipe_lists_on_a_strided_layout(S, dev):
    """The recipe's lists (tools/lvd_step.py RECIPE_TARGET) on Nl = 20, the layout passed as the slice ``inp[:, :, 3:]``
    of a 23-channel clip as LvdStep passes it: the bits of its contiguous copy, and the restatement's values."""
    from waldo_amd.tools.lvd_step import RECIPE_TARGET
    flow, clip = SR.recipe_clip(40, 72)
    inp = clip.to(dev)
    view = inp[:, :, 3:]
    assert view.shape[2] == 20 and not view.is_contiguous()
    lyt = clip[:, :, 3:].contiguous()
    lists = tuple(RECIPE_TARGET[name] for name in ("fg_idx", "bg_idx", "other_idx"))
    thresh = {name: RECIPE_TARGET[name] for name in THRESH}
    opts = {name: v for name, v in RECIPE_TARGET.items() if name not in thresh and not name.endswith("_idx")}
    assert opts == dict(reg_bg_mul=0.25, use_fg=True, use_dominant_flow_other=True)
    both = (R.moving_object_target(flow, lyt, **RECIPE_TARGET),
            R.moving_object_target(flow.double(), lyt.double(), **RECIPE_TARGET))
    # every field of the STRIDED call against the restatement (the candidate is handed the view, whatever it is passed)
    a = check_target(lambda f, _, *ls, **kw: S.moving_object_target(f.to(dev), view, *ls, **kw), flow, lyt, lists, thresh,
                     lambda **kw: both, opts, "Nl=20 strided")
    b = S.moving_object_target(flow.to(dev), view.contiguous(), **RECIPE_TARGET)
    for name, x, y in zip(a._fields, a, b):
        assert torch.equal(x, y), name


def test_moving_object_target_keeps_the_nan_of_a_listed_other_channel(S, dev):
    """use_dominant_flow_other: ``torch.max(mask, other_prop * dominant_flow * flow_edge)`` returns NaN where either side
    is one.  A NaN planted in the listed ``other`` channel at five pixels -- in both blur tile rows, the last pixel of
    a frame among them -- comes out in mov_obj_mask and mov_obj there and nowhere else."""
    flow, lyt, lists, thresh, _ = SR.target_refs(40, 72, 15)
    lyt = lyt.clone()
    planted = [(0, 0, 0, 0), (0, 2, 17, 40), (1, 0, 33, 70), (1, 1, 39, 71), (1, 2, 5, 64)]
    for b, t, y, x in planted:
        lyt[b, t, lists[2][0], y, x] = float("nan")
    r32 = R.moving_object_target(flow, lyt, *lists, **thresh, **SR.RECIPE_OPTS)
    r64 = R.moving_object_target(flow.double(), lyt.double(), *lists, **thresh, **SR.RECIPE_OPTS)
    got = S.moving_object_target(flow.to(dev), lyt.to(dev), *lists, **thresh, **SR.RECIPE_OPTS)
    want = torch.isnan(r32["mov_obj_mask"])
    assert int(want.sum()) == len(planted) and all(want[b, t, 0, y, x] for b, t, y, x in planted)
    assert torch.equal(torch.isnan(r64["mov_obj_mask"]), want) and torch.equal(torch.isnan(r32["mov_obj"]), want)
    assert torch.equal(torch.isnan(got.mov_obj_mask).cpu(), want) and torch.equal(torch.isnan(got.mov_obj).cpu(), want)
    for name in ("fg_prop", "mean_bg_flow", "flow_edge", "dominant_flow"):
        assert not torch.isnan(getattr(got, name)).any(), name
    quantities = list(deciding(r32, r64, thresh))
    for name in ("mov_obj_mask", "mov_obj"):
        decisions(getattr(got, name).nan_to_num(0.0), r32[name].nan_to_num(0.0), quantities, f"{name} beside the NaNs")


# ---------------------------------------------------------------------------------------------------------------------
# cell distance
# ---------------------------------------------------------------------------------------------------------------------
def cell_inputs(no, obj_shape, h, w, mask, seed=0):
    g = torch.Generator().manual_seed(seed)
    lo = obj_shape[0] * obj_shape[1]
    pose = 0.6 * torch.randn(2, 3, no, lo, 2, generator=g)
    fg = 1.2 * torch.rand(2, 3, 1, h, w, generator=g)   # some weights (1 - fg) are negative
    return pose, fg, mask[..., :h, :w].contiguous()


def hip_cell(S, dev, pose, fg, m, obj_shape, eps, center=True):
    p, f = pose.to(dev).requires_grad_(), fg.to(dev).requires_grad_()
    out = S.cell_distance(p, obj_shape, m.to(dev), f, eps=eps, center=center)
    if not center:
        gp, gf = torch.autograd.grad(out, [p, f])
        return out.detach(), None, gp, gf, None
    cell, centre = out
    gp, gf = torch.autograd.grad(cell, [p, f], retain_graph=True)
    gpc, = torch.autograd.grad(centre, [p])
    return cell.detach(), centre.detach(), gp, gf, gpc


def device_cell(S, dev):
    return lambda *a, **kw: hip_cell(S, dev, *a, **kw)


def check_cell(cell, pose, fg, m, obj_shape, what):
    """``cell(pose, fg, m, obj_shape, eps, center=True)`` -> (cell_dis, center_dis, grad pose, grad fg_mask, grad pose of
    center_dis) against the restatement at eps 0 and 0.1, and the ``center=False`` call against the bits of the other.
    The references are computed once per operands (supervision_regimes.cell_refs).  Returns the results per eps."""
    out = []
    for eps in (0.0, 0.1):
        r32, r64 = SR.cell_refs(pose, fg, m, obj_shape, eps)
        got = cell(pose, fg, m, obj_shape, eps)
        names = ("cell_dis", "center_dis", "grad_pose", "grad_fg_mask", "grad_pose (center)")
        for name, a, b, e in zip(names, got, r32, r64):
            close(a.reshape(-1) if a.ndim == 0 else a, b.reshape(-1) if b.ndim == 0 else b, rel=True,
                  what=f"{name} {what} eps={eps}", exact=e.reshape(-1) if e.ndim == 0 else e)
        alone = cell(pose, fg, m, obj_shape, eps, center=False)
        assert torch.equal(alone[0], got[0]) and torch.equal(alone[2], got[2]) and torch.equal(alone[3], got[3])
        out.append(got)
    return out


OLD_CELL_CASES = [(no, obj_shape, h, w) for h, w in ((24, 40), (17, 33))
                  for no, obj_shape in ((1, (2, 2)), (5, (4, 4)), (16, (4, 4)), (3, (2, 3)))]


def old_cell_operands(refs, no, obj_shape, h, w):
    mask = refs(use_fg=True, use_dominant_flow_other=True)[0]["mov_obj_mask"]
    pose, fg, m = cell_inputs(no, obj_shape, h, w, mask, seed=no)
    assert 0.1 < (m > 0).float().mean().item() < 0.9 and (fg > 1).any()
    return pose, fg, m


@pytest.mark.parametrize("no,obj_shape", [(1, (2, 2)), (5, (4, 4)), (16, (4, 4)), (3, (2, 3))])
@pytest.mark.parametrize("h,w", [(24, 40), (17, 33)])
def test_cell_distance(S, dev, target_case, no, obj_shape, h, w):
    """B T = 6; 24 x 40 and the odd 17 x 33 (one partial workgroup per frame); the mask is the target test's."""
    pose, fg, m = old_cell_operands(target_case[2], no, obj_shape, h, w)
    check_cell(device_cell(S, dev), pose, fg, m, obj_shape, f"No={no} {obj_shape} {h}x{w}")


def tie_operands(refs):
    pose, fg, m = cell_inputs(3, (4, 4), 24, 40, refs()[0]["mov_obj_mask"], seed=4)
    pose[:, :, 2] = pose[:, :, 0]
    return pose, fg, m


def check_cell_ties(cell, pose, fg, m):
    for eps in (0.0, 0.1):
        got = cell(pose, fg, m, (4, 4), eps)
        r32, r64 = SR.cell_refs(pose, fg, m, (4, 4), eps)
        for g in (got[2], got[4], r32[2], r32[4]):
            assert (g[:, :, 2] == 0).all() and (g[:, :, 0] != 0).any()
        close(got[2], r32[2], rel=True, what=f"grad_pose, planted tie, eps={eps}", exact=r64[2])
        close(got[4], r32[4], rel=True, what=f"grad_pose (center), planted tie, eps={eps}", exact=r64[4])


def test_cell_distance_ties_go_to_the_lowest_index(S, dev, target_case):
    """Two objects with identical poses: the lower index takes the whole gradient, as torch.min(dim) gives it on the CPU."""
    check_cell_ties(device_cell(S, dev), *tie_operands(target_case[2]))


@pytest.mark.parametrize("case", SR.CELL_CASES, ids=lambda c: "B{}T{}No{}_{}x{}_{}x{}".format(*c[:3], *c[3], *c[4:]))
def test_cell_distance_across_chunks(S, dev, case):
    """More than one chunk of 2048 pixels per frame, a ragged last chunk, 31 objects, more than 256 partials
    (supervision_regimes.CELL_CASES): values and gradients against the restatement, the bits of the call without the
    centre term, and the same bits from a second run in either deterministic mode."""
    import waldo_amd
    b, t, no, obj_shape, h, w = case
    pose, fg, m = SR.cell_inputs(*case, seed=SR.cell_seed(case))
    got = check_cell(device_cell(S, dev), pose, fg, m, obj_shape, f"B={b} T={t} No={no} {obj_shape} {h}x{w}")
    for eps, first in zip((0.0, 0.1), got):
        for mode in (False, False, True, True):
            with waldo_amd.deterministic(mode):
                again = hip_cell(S, dev, pose, fg, m, obj_shape, eps)
            for x, y in zip(first, again):
                assert torch.equal(x, y), (eps, mode)


def test_cell_distance_refuses_32_objects_on_the_device(S, dev):
    pose, fg, m = SR.cell_inputs(2, 3, 32, (4, 4), 33, 70, seed=1)
    with pytest.raises(ValueError, match="No = 32"):
        S.cell_distance(pose.to(dev), (4, 4), m.to(dev), fg.to(dev))
    from waldo_amd import _lib
    assert _lib.query("waldo_cell_distance_workspace_bytes", 6, 32, 33 * 70) == 0


def test_cell_distance_is_bit_reproducible_in_both_modes(S, dev, target_case):
    import waldo_amd
    mask = target_case[2]()[0]["mov_obj_mask"]
    pose, fg, m = cell_inputs(16, (4, 4), 24, 40, mask, seed=9)
    runs = []
    for mode in (False, False, True, True):
        with waldo_amd.deterministic(mode):
            runs.append(hip_cell(S, dev, pose, fg, m, (4, 4), 0.1))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_cell_distance_keeps_no_per_cell_tensor(S, dev):
    """64 x 128, 16 objects of 4 x 4 points, 6 frames: the reference's (B, T, No, 9, H, W) tensor would be 28 MB; forward and
    backward together stay under 4 MB above their inputs and outputs."""
    g = torch.Generator().manual_seed(2)
    pose = (0.6 * torch.randn(2, 3, 16, 16, 2, generator=g)).to(dev).requires_grad_()
    fg = (1.2 * torch.rand(2, 3, 1, 64, 128, generator=g)).to(dev).requires_grad_()
    m = (torch.rand(2, 3, 1, 64, 128, generator=g) > 0.5).float().to(dev)
    S.cell_distance(pose.detach(), (4, 4), m, fg.detach())  # (the pixel axes are made once per size: not this call's)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = S.cell_distance(pose, (4, 4), m, fg, eps=0.1)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = pose.grad.numel() * 4 + fg.grad.numel() * 4 + 512
    print(f"[cell_distance] peak above the inputs {peak} bytes, outputs {outputs} bytes")
    assert peak - outputs < 4 * 2 ** 20, (peak, outputs)
    assert 6 * 16 * 9 * 64 * 128 * 4 > 28e6


# ---------------------------------------------------------------------------------------------------------------------
# the recipe's objective and LvdStep
# ---------------------------------------------------------------------------------------------------------------------
def recipe_leaves(flow, h, w):
    """alpha_flt (No = 5 objects and the background), rec_flow and obj_pose of the recipe's objective at h x w."""
    g = torch.Generator().manual_seed(21)
    alpha = 2 * torch.softmax(torch.randn(2, 3, 6, h, w, generator=g), dim=2) - 1
    rec_flow = flow[:, 1:] + 0.01 * torch.randn(2, 2, 2, h, w, generator=g)
    pose = 0.6 * torch.randn(2, 3, 5, 16, 2, generator=g)
    return alpha, rec_flow, pose


def test_recipe_terms(S, dev, target_case):
    """The four scalars and the gradients on alpha_flt, rec_flow and obj_pose at 24 x 40.  Both sides get the SAME target
    (the device's: the target has its tests above), so that what is compared is the objective."""
    check_recipe_terms(S, dev, target_case[0], target_case[1], THRESH, 24, 40)


def test_recipe_terms_across_chunks(S, dev):
    """40 x 72: two chunks of ``cell_dis``, four tiles of the edge mask's blur."""
    flow, lyt, _, thresh, _ = SR.target_refs(40, 72, 15)
    check_recipe_terms(S, dev, flow, lyt, thresh, 40, 72)


def check_recipe_terms(S, dev, flow, lyt, thresh, h, w):
    opts = dict(use_fg=True, use_dominant_flow_other=True)
    tgt = S.moving_object_target(flow.to(dev), lyt.to(dev), FG, BG, OTHER, **thresh, **opts)
    alpha, rec_flow, pose = recipe_leaves(flow, h, w)

    def run(fn, cast, target):
        leaves = [cast(x).requires_grad_() for x in (alpha, rec_flow, pose)]
        terms = fn(leaves[0], leaves[1], cast(flow), cast(lyt), leaves[2], (4, 4), target, cell_dis_eps=0.1)
        total = 10 * terms["cell_dis"] + 1000 * terms["l1_flow"] + 10 * terms["reg_mov"] + terms["ent_flt_edge"]
        return {k: v.detach() for k, v in terms.items()}, torch.autograd.grad(total, leaves)

    got_t, got_g = run(S.recipe_terms, lambda x: x.to(dev), tgt)
    refs = []
    for dtype in (torch.float32, torch.float64):
        target = {k: getattr(tgt, k).cpu().to(dtype) for k in ("mov_obj_mask", "mov_obj")}
        refs.append(run(R.recipe_terms, lambda x: x.to(dtype), target))
    (t32, g32), (t64, g64) = refs
    assert set(got_t) == {"cell_dis", "reg_mov", "ent_flt_edge", "l1_flow"}
    for name in got_t:
        assert t32[name].abs().item() > 1e-4, name
        close(got_t[name].reshape(1), t32[name].reshape(1), rel=True, what=name, exact=t64[name].reshape(1))
    for name, a, b, e in zip(("grad alpha_flt", "grad rec_flow", "grad obj_pose"), got_g, g32, g64):
        assert b.abs().max().item() > 0
        close(a, b, rel=True, what=name, exact=e)


def test_the_step_path_reads_nothing_on_the_host(S, dev):
    """After one call at the size (the pixel axes are copied to the device on first use), the target, ``cell_distance``
    forward and backward and ``recipe_terms`` synchronise with nothing: under ``set_sync_debug_mode("error")`` a host
    read of a device value -- an ``item()``, a boolean index, a copy to the host -- raises."""
    flow, lyt, lists, thresh, _ = SR.target_refs(40, 72, 15)
    alpha, rec_flow, pose = (x.to(dev) for x in recipe_leaves(flow, 40, 72))
    flow, lyt = flow.to(dev), lyt.to(dev)

    def step():
        tgt = S.moving_object_target(flow, lyt, *lists, **thresh, **SR.RECIPE_OPTS)
        leaves = [x.detach().clone().requires_grad_() for x in (alpha, rec_flow, pose)]
        fg_mask = ((leaves[0][:, :, 1:] + 1) / 2).sum(dim=2, keepdim=True)
        cell, centre = S.cell_distance(leaves[2], (4, 4), tgt.mov_obj_mask, fg_mask, eps=0.1, center=True)
        (cell + centre).backward()
        terms = S.recipe_terms(leaves[0], leaves[1], flow, lyt, leaves[2], (4, 4), tgt, cell_dis_eps=0.1)
        sum(terms.values()).backward()
        return [x.grad for x in leaves]

    warm = step()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        grads = step()
        with pytest.raises(RuntimeError):   # the mode is live here: the read this test is about does raise
            grads[0].sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for a, b in zip(warm, grads):
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_lvd_step_with_the_recipe_objective(dev):
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(1, dev, objective="recipe")
    loss = step()
    assert torch.isfinite(loss).item() and step.grads_finite()
    assert set(step.terms) == {"cell_dis", "reg_mov", "ent_flt_edge", "l1_flow"}
    assert all(torch.isfinite(v).item() for v in step.terms.values())
    assert all(x.grad is not None and x.grad.abs().max().item() > 0 for x in (step.raw, step.pose_o, step.score))


def test_lvd_step_default_objective_is_unchanged(dev):
    """The default objective is the stand-in of before, on the same seeded leaves: the loss has the bits of the stand-in
    expression evaluated here on the step's own tensors, and the recipe mode draws its flow AFTER every leaf."""
    from waldo_amd.nets import decode_output, estimate_alpha_grid_occ, flp
    from waldo_amd.nets.lvd import decoder_tail
    from waldo_amd.tools.lvd_step import LvdStep
    s = LvdStep(1, dev)
    assert s.objective == "stand-in" and s.real_flow is None
    loss = s()
    b, t, no, lo, lb, ho = s.shape
    obj_alpha = decoder_tail(s.raw, init_bias=5.0).view(b, no, 1, ho, ho)   # LvdStep.__call__'s forward, line for line
    obj_pose = flp.obj_pose_to_points(torch.tanh(s.pose_o), s.base_o, s.mul6, s.bias_o, 0.2)
    bg_pose = flp.bg_pose_to_points(torch.tanh(s.pose_b), s.base_b, s.bias_b, 1.2)
    occ, oa, ba, grid = estimate_alpha_grid_occ(s.warper, obj_alpha, s.bg_alpha, obj_pose.view(b, t, no, lo, 2),
                                                bg_pose.view(b, t, 1, lb, 2), s.score)
    out = decode_output(s.warper, s.inp, grid, occ, oa, ba, s.cls_logit.softmax(-1), s.ctx_ts, s.pred_ts,
                        restrict_to_ctx=False)
    want = out[0].square().mean() + out[1].square().mean() + out[3].mean()
    assert torch.equal(loss.detach(), want.detach()), (loss.item(), want.item())
    r = LvdStep(1, dev, objective="recipe")
    for a, b_ in zip(s.leaves + [s.inp], r.leaves + [r.inp]):
        assert torch.equal(a, b_)
