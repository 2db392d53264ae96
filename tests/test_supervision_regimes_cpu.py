"""CPU: the fixtures of tests/supervision_regimes.py are what the GPU cases built on them assume -- checked on the
restatement alone (tests/supervision_ref.py), with the yardsticks of tests/test_gpu_supervision.py.

A target fixture must populate both sides of every threshold, keep the pixels within the decision margin (16 x the fp32
noise) and the fp32 / fp64 flips under HALF the 0.5 % cap that ``decisions`` grants, and take the ``== 0`` branch of the
blurred weight on frame (0, 1) only.  A ``cell_distance`` fixture must put mask pixels and at least two chosen objects
into EVERY chunk of 2048 pixels of every frame: a wrong chunk index then moves the result."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import supervision_regimes as SR  # noqa: E402
import test_gpu_supervision as G  # noqa: E402


def first_fixture():
    """The 24 x 40 fixture as tests/test_gpu_supervision.py built it before ``target_inputs`` took a size, line for line."""
    nl = 6
    g = torch.Generator().manual_seed(7)
    cls = torch.randint(0, nl, (2, 3, 6, 10), generator=g).repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)
    cls[0, 1] = 0
    lyt = torch.nn.functional.one_hot(cls, nl).permute(0, 1, 4, 2, 3).float() * 10 - 5
    lyt[1, 2] = 10 * torch.softmax(2 * torch.randn(nl, 24, 40, generator=g), dim=0) - 5
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, 24), torch.linspace(-1, 1, 40), indexing="ij")
    flow = torch.stack([0.012 * torch.sin(2 * xs + ys), 0.008 * torch.cos(1.5 * ys - xs)]).expand(2, 3, 2, 24, 40).clone()
    flow *= torch.linspace(0.6, 1.4, 6).view(2, 3, 1, 1, 1)
    flow[:, :, 0, 6:17, 10:26] += 0.03
    flow[:, :, 1, 6:17, 10:26] -= 0.02
    flow += 5e-4 * torch.randn(flow.shape, generator=g)
    return flow.contiguous(), lyt.contiguous()


def test_the_24_x_40_fixture_kept_its_bits():
    """``target_inputs`` generalises the fixture the GPU file was written with; at 24 x 40 it returns that one."""
    flow, lyt = SR.target_inputs(24, 40)
    was = first_fixture()
    assert torch.equal(flow, was[0]) and torch.equal(lyt, was[1])
    assert G.target_inputs is SR.target_inputs and torch.equal(SR.target_refs()[0], was[0])


@pytest.mark.parametrize("h,w,edge_size", SR.TARGET_CASES)
def test_target_fixtures_populate_both_sides_of_every_threshold(h, w, edge_size):
    _, _, _, thresh, refs = SR.target_refs(h, w, edge_size)
    G.check_target_fixture(refs, thresh, f"{h}x{w} e={edge_size}")


def test_the_32_channel_fixture_is_the_six_channel_one_moved():
    _, _, _, thresh, wide = SR.target_refs(40, 72, 15, layout="wide")
    six = SR.target_refs(40, 72, 15)[4]
    G.check_target_fixture(wide, thresh, "40x72 Nl=32")
    for name in ("fg_prop", "nobg_prop", "mov_obj_mask"):
        assert torch.equal(wide()[0][name], six()[0][name]), name


def test_the_recipe_clip_populates_the_recipes_thresholds():
    """Nl = 20 with the recipe's lists: the parity checks of the strided case need few pixels near a threshold too."""
    from waldo_amd.tools.lvd_step import RECIPE_TARGET
    from supervision_ref import moving_object_target
    flow, clip = SR.recipe_clip(40, 72)
    lyt = clip[:, :, 3:].contiguous()
    r32, r64 = moving_object_target(flow, lyt, **RECIPE_TARGET), moving_object_target(flow.double(), lyt.double(),
                                                                                      **RECIPE_TARGET)
    assert 0.1 <= r32["mov_obj_mask"].mean().item() <= 0.9
    assert (lyt[:, :, 9] > 0).any()            # the listed ``other`` channel is present
    for q32, q64 in G.deciding(r32, r64, RECIPE_TARGET):
        noise = (q32.double() - q64).abs().max().item()
        near = (q64.abs() <= G.MARGIN_X * noise).float().mean().item()
        flips = ((q32 > 0) != (q64 > 0)).float().mean().item()
        print(f"[recipe clip] fp32 noise {noise:.3e}, {near:.5f} within the margin, {flips:.5f} flipped")
        assert near <= G.EXCUSED / 2 and flips <= G.EXCUSED / 2


@pytest.mark.parametrize("case", SR.CELL_CASES, ids=str)
def test_cell_fixtures_fill_every_chunk(case):
    b, t, no, obj_shape, h, w = case
    pose, fg, m = SR.cell_inputs(*case, seed=SR.cell_seed(case))
    assert (fg > 1).any()
    hw = h * w
    chunks = -(-hw // SR.CELL_CHUNK)
    assert chunks >= 2
    fewest_mask, fewest_objects = hw, no
    for eps in (0.0, 0.1):
        chosen = SR.chosen_objects(pose, fg, m, obj_shape, eps)
        for f in range(b * t):
            for c in range(chunks):
                px = slice(c * SR.CELL_CHUNK, min((c + 1) * SR.CELL_CHUNK, hw))
                on = m.view(b * t, hw)[f, px] > 0
                fewest_mask = min(fewest_mask, int(on.sum()))
                # eps = 0: a pixel off the mask has weight 0, every object ties there -- count the masked pixels only
                fewest_objects = min(fewest_objects, chosen[f, px][on].unique().numel())
    print(f"[cell fixture] {case}: {chunks} chunks, at least {fewest_mask} mask pixels and {fewest_objects} different "
          f"objects chosen in every (frame, chunk)")
    assert fewest_mask > 0 and fewest_objects >= min(2, no)
    if no == 31:                               # the last object is chosen somewhere: a minimum that stops early shows
        assert (SR.chosen_objects(pose, fg, m, obj_shape, 0.1) == 30).any()
