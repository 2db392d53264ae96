"""GPU: waldo_amd.supervision against its restatement in framework ops (tests/supervision_ref.py) in fp32 and fp64, and
against the fixture recorded from the reference's EdgeExtractor (tests/golden/flow_edges_reference.npz).

Continuous outputs go through tests/parity.py::close.  A 0 / 1 map is a threshold decision: a pixel may differ from the
fp32 restatement only where the fp64 restatement's DECIDING quantity (flow_edge - flow_thresh, delta_flow -
mov_obj_thresh, sum flow^2 - sum mean^2) lies within a margin of zero; the margin is 16 x the largest |fp32 - fp64| of that
quantity, measured here and printed, and at most 0.5 % of the pixels may be excused that way (``decisions``)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import supervision_ref as R  # noqa: E402
from parity import TOL, close  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_X, EXCUSED = 16.0, 0.005
FG, BG, OTHER, NL = [0, 3], [1, 2], [4], 6           # (channel 5 is in no list)
THRESH = dict(flow_thresh=0.02, mov_obj_thresh=0.005, blur_sigma=2.0, edge_size=7)


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


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian blur
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 23])
@pytest.mark.parametrize("c", [1, 3, 20])
@pytest.mark.parametrize("h,w", [(24, 40), (12, 70)])
def test_gaussian_blur(S, dev, k, c, h, w):
    """12 x 70: pad 11 against height 12, two tile columns; 24 x 40: no multiple of the 32 x 64 tile."""
    g = torch.Generator().manual_seed(100 * k + c)
    x = torch.randn(2, c, h, w, generator=g)
    got = S.gaussian_blur(x.to(dev), 2.0, k)
    assert got.shape == x.shape
    close(got, R.gaussian_blur(x, 2.0, k), what=f"blur k={k} C={c} {h}x{w}", exact=R.gaussian_blur(x.double(), 2.0, k))


def test_gaussian_blur_keeps_leading_dimensions_and_a_constant(S, dev):
    x = torch.full((2, 3, 2, 24, 40), 0.37, device=dev)
    got = S.gaussian_blur(x, 3.0)
    assert got.shape == x.shape and (got - 0.37).abs().max().item() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# moving-object target
# ---------------------------------------------------------------------------------------------------------------------
def target_inputs():
    """2 x 3 frames at 24 x 40.  Layouts: one-hot +-5 in 4 x 4 blocks; frame (0, 1) all foreground (class 0: the blurred
    weight is exactly 0); frame (1, 2) soft.  Flow: smooth, plus a rectangle that moves on its own, plus noise of 5e-4."""
    g = torch.Generator().manual_seed(7)
    cls = torch.randint(0, NL, (2, 3, 6, 10), generator=g).repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)
    cls[0, 1] = 0
    lyt = torch.nn.functional.one_hot(cls, NL).permute(0, 1, 4, 2, 3).float() * 10 - 5
    lyt[1, 2] = 10 * torch.softmax(2 * torch.randn(NL, 24, 40, generator=g), dim=0) - 5
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, 24), torch.linspace(-1, 1, 40), indexing="ij")
    flow = torch.stack([0.012 * torch.sin(2 * xs + ys), 0.008 * torch.cos(1.5 * ys - xs)]).expand(2, 3, 2, 24, 40).clone()
    flow *= torch.linspace(0.6, 1.4, 6).view(2, 3, 1, 1, 1)
    flow[:, :, 0, 6:17, 10:26] += 0.03
    flow[:, :, 1, 6:17, 10:26] -= 0.02
    flow += 5e-4 * torch.randn(flow.shape, generator=g)
    return flow.contiguous(), lyt.contiguous()


@pytest.fixture(scope="module")
def target_case():
    """The inputs and the restatement's targets (fp32, fp64) per option set, each computed once."""
    flow, lyt = target_inputs()
    cache = {}

    def refs(**opts):
        key = tuple(sorted(opts.items()))
        if key not in cache:
            cache[key] = (R.moving_object_target(flow, lyt, FG, BG, OTHER, **THRESH, **opts),
                          R.moving_object_target(flow.double(), lyt.double(), FG, BG, OTHER, **THRESH, **opts))
        return cache[key]

    return flow, lyt, refs


def test_target_fixture_populates_both_sides_of_every_threshold(target_case):
    flow, lyt, refs = target_case
    r = refs()[0]
    for name, frac in (("flow_edge", r["flow_edge"].mean().item()), ("dominant_flow", r["dominant_flow"].mean().item()),
                       ("mov_obj_mask", r["mov_obj_mask"].mean().item()),
                       ("fg_prop > 0", (r["fg_prop"] > 0).float().mean().item()),
                       ("nobg_prop > 0", (r["nobg_prop"] > 0).float().mean().item())):
        print(f"[target fixture] {name}: {frac:.3f} of the pixels")
        assert 0.1 <= frac <= 0.9, (name, frac)
    # the restatement alone stays far inside the cap: few pixels of THIS fixture sit within the margin of a threshold
    r32, r64 = refs()
    for name, thresh in (("edge_raw", THRESH["flow_thresh"]), ("delta_flow", THRESH["mov_obj_thresh"]),
                         ("dominant_margin", 0.0)):
        noise = (r32[name].double() - r64[name]).abs().max().item()
        near = ((r64[name] - thresh).abs() <= MARGIN_X * noise).float().mean().item()
        flips = ((r32[name] > thresh) != (r64[name] > thresh)).float().mean().item()
        print(f"[target fixture] {name}: fp32 noise {noise:.3e}, {near:.5f} of the pixels within {MARGIN_X:g} x of it, "
              f"{flips:.5f} decided differently in fp32 and fp64")
        assert near <= EXCUSED / 2 and flips <= EXCUSED / 2, name
    blurred0 = R.gaussian_blur(1 - r["fg_prop"], THRESH["blur_sigma"])
    assert (blurred0[0, 1] == 0).all() and (blurred0[0, 0] != 0).any()  # the `== 0` branch runs, and not everywhere


OPTION_SETS = [dict(), dict(use_fg=True), dict(use_nobg=True), dict(use_nobg_edge=True, nobg_edge_mul=0.3),
               dict(use_flow_nobg=True), dict(use_dominant_flow_other=True), dict(reg_bg_mul=0.0),
               dict(use_fg=True, use_dominant_flow_other=True),                                          # the recipe's
               dict(use_fg=True, use_nobg=True, use_nobg_edge=True, nobg_edge_mul=-0.5, use_flow_nobg=True)]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "+".join(k for k in o) or "plain")
def test_moving_object_target(S, dev, target_case, opts):
    flow, lyt, refs = target_case
    r32, r64 = refs(**opts)
    got = S.moving_object_target(flow.to(dev), lyt.to(dev), FG, BG, OTHER, **THRESH, **opts)
    what = "+".join(opts) or "plain"
    for name in got._fields:
        assert getattr(got, name).shape == r32[name].shape and not getattr(got, name).requires_grad, name
    close(got.fg_prop, r32["fg_prop"], what=f"fg_prop {what}", exact=r64["fg_prop"])
    close(got.mean_bg_flow, r32["mean_bg_flow"], what=f"mean_bg_flow {what}", exact=r64["mean_bg_flow"])
    assert (got.mean_bg_flow[0, 1] == 0).all()
    edge = (r32["edge_raw"] - THRESH["flow_thresh"], r64["edge_raw"] - THRESH["flow_thresh"])
    delta = (r32["delta_flow"] - THRESH["mov_obj_thresh"], r64["delta_flow"] - THRESH["mov_obj_thresh"])
    dominant = (r32["dominant_margin"], r64["dominant_margin"])
    decisions(got.flow_edge, r32["flow_edge"], [edge], f"flow_edge {what}")
    decisions(got.dominant_flow, r32["dominant_flow"], [dominant], f"dominant_flow {what}")
    decisions(got.mov_obj_mask, r32["mov_obj_mask"], [edge, delta, dominant], f"mov_obj_mask {what}")
    decisions(got.mov_obj, r32["mov_obj"], [edge, delta, dominant], f"mov_obj {what}")


def test_moving_object_target_accepts_frames_without_a_clip_dimension(S, dev, target_case):
    flow, lyt, refs = target_case
    a = S.moving_object_target(flow.to(dev), lyt.to(dev), FG, BG, OTHER, **THRESH, use_fg=True)
    b = S.moving_object_target(flow.view(6, 2, 24, 40).to(dev), lyt.view(6, NL, 24, 40).to(dev), FG, BG, OTHER, **THRESH,
                               use_fg=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(y.shape), y)


# ---------------------------------------------------------------------------------------------------------------------
# cell distance
# ---------------------------------------------------------------------------------------------------------------------
def cell_inputs(no, obj_shape, h, w, mask, seed=0):
    g = torch.Generator().manual_seed(seed)
    lo = obj_shape[0] * obj_shape[1]
    pose = 0.6 * torch.randn(2, 3, no, lo, 2, generator=g)
    fg = 1.2 * torch.rand(2, 3, 1, h, w, generator=g)   # some weights (1 - fg) are negative
    return pose, fg, mask[..., :h, :w].contiguous()


def ref_cell(pose, fg, m, obj_shape, eps, dtype):
    p, f = pose.to(dtype).requires_grad_(), fg.to(dtype).requires_grad_()
    cell, centre = R.cell_distance(p, obj_shape, m.to(dtype), f, eps)
    gp, gf = torch.autograd.grad(cell, [p, f], retain_graph=True)
    gpc, = torch.autograd.grad(centre, [p])
    return cell.detach(), centre.detach(), gp, gf, gpc


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


@pytest.mark.parametrize("no,obj_shape", [(1, (2, 2)), (5, (4, 4)), (16, (4, 4)), (3, (2, 3))])
@pytest.mark.parametrize("h,w", [(24, 40), (17, 33)])
def test_cell_distance(S, dev, target_case, no, obj_shape, h, w):
    """B T = 6; 24 x 40 and the odd 17 x 33 (one partial workgroup per frame); the mask is the target test's."""
    mask = target_case[2](use_fg=True, use_dominant_flow_other=True)[0]["mov_obj_mask"]
    pose, fg, m = cell_inputs(no, obj_shape, h, w, mask, seed=no)
    assert 0.1 < (m > 0).float().mean().item() < 0.9 and (fg > 1).any()
    for eps in (0.0, 0.1):
        r32, r64 = ref_cell(pose, fg, m, obj_shape, eps, torch.float32), ref_cell(pose, fg, m, obj_shape, eps, torch.float64)
        got = hip_cell(S, dev, pose, fg, m, obj_shape, eps)
        names = ("cell_dis", "center_dis", "grad_pose", "grad_fg_mask", "grad_pose (center)")
        for name, a, b, e in zip(names, got, r32, r64):
            close(a.reshape(-1) if a.ndim == 0 else a, b.reshape(-1) if b.ndim == 0 else b, rel=True,
                  what=f"{name} No={no} {obj_shape} {h}x{w} eps={eps}", exact=e.reshape(-1) if e.ndim == 0 else e)
        alone = hip_cell(S, dev, pose, fg, m, obj_shape, eps, center=False)
        assert torch.equal(alone[0], got[0]) and torch.equal(alone[2], got[2]) and torch.equal(alone[3], got[3])


def test_cell_distance_ties_go_to_the_lowest_index(S, dev, target_case):
    """Two objects with identical poses: the lower index takes the whole gradient, as torch.min(dim) gives it on the CPU."""
    mask = target_case[2]()[0]["mov_obj_mask"]
    pose, fg, m = cell_inputs(3, (4, 4), 24, 40, mask, seed=4)
    pose[:, :, 2] = pose[:, :, 0]
    for eps in (0.0, 0.1):
        got = hip_cell(S, dev, pose, fg, m, (4, 4), eps)
        r32, r64 = ref_cell(pose, fg, m, (4, 4), eps, torch.float32), ref_cell(pose, fg, m, (4, 4), eps, torch.float64)
        for g in (got[2], got[4], r32[2], r32[4]):
            assert (g[:, :, 2] == 0).all() and (g[:, :, 0] != 0).any()
        close(got[2], r32[2], rel=True, what=f"grad_pose, planted tie, eps={eps}", exact=r64[2])
        close(got[4], r32[4], rel=True, what=f"grad_pose (center), planted tie, eps={eps}", exact=r64[4])


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
def test_recipe_terms(S, dev, target_case):
    """The four scalars and the gradients on alpha_flt, rec_flow and obj_pose at 24 x 40.  Both sides get the SAME target
    (the device's: the target has its tests above), so that what is compared is the objective."""
    flow, lyt, _ = target_case
    opts = dict(use_fg=True, use_dominant_flow_other=True)
    tgt = S.moving_object_target(flow.to(dev), lyt.to(dev), FG, BG, OTHER, **THRESH, **opts)
    g = torch.Generator().manual_seed(21)
    alpha = 2 * torch.softmax(torch.randn(2, 3, 6, 24, 40, generator=g), dim=2) - 1
    rec_flow = flow[:, 1:] + 0.01 * torch.randn(2, 2, 2, 24, 40, generator=g)
    pose = 0.6 * torch.randn(2, 3, 5, 16, 2, generator=g)

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
