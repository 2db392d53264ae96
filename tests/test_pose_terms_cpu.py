"""CPU: ``supervision.pose_terms``' framework route (the masked sum that reads nothing on the host) against the
reference's spelling (tests/pose_terms_ref.py) in fp32 and fp64 -- values and autograd gradients in ``pred`` and
``real`` --, its refusals, and a tiny ``FlpStep`` on the CPU."""
import pytest
import torch

import pose_terms_ref as R
from parity import close

SHAPES = [(2, 3, 3, 4, 6), (3, 5, 5, 4, 8)]


def _framework(real, pred, ctx_mask):
    from waldo_amd import supervision as S
    return S.pose_terms(real, pred, ctx_mask, fused=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind", [k for k in R.MASKS if k != "all"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_framework_route_equals_the_references_spelling(shape, kind, dtype):
    real, pred = R.inputs(*shape)
    m = R.mask(kind, *shape[:2])
    if kind == "holes":
        counts = m.sum(dim=1).tolist()
        assert len(set(counts)) == len(counts) and not m[:, 0].any() and m[:, 1].all()
    got = R.terms_and_grads(_framework, real, pred, m, dtype=dtype)
    ref = R.terms_and_grads(R.pose_terms, real, pred, m, dtype=dtype)
    exact = R.terms_and_grads(R.pose_terms, real, pred, m, dtype=torch.float64)
    for k in R.NAMES:
        assert got[0][k].ndim == 0 and got[0][k].dtype == dtype
        close(got[0][k], ref[0][k], rel=True, exact=exact[0][k], what=f"{kind} {k}")
    for side, name in ((1, "real"), (2, "pred")):
        for i, k in enumerate(R.NAMES):
            close(got[side][i], ref[side][i], rel=True, exact=exact[side][i], what=f"{kind} grad {name} {k}")
            assert (got[side][i][m] == 0).all(), (kind, name, k)                      # context frames: exact zeros
            planted = (torch.arange(real[i].numel()) % 5 == 0).view(real[i].shape)
            assert (got[side][i][planted] == 0).all(), (kind, name, k)               # sgn(0) = 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_an_all_context_mask_gives_nan_terms_and_zero_gradients(dtype):
    real, pred = R.inputs(*SHAPES[0])
    m = R.mask("all", *SHAPES[0][:2])
    ref = R.pose_terms(real, pred, m)
    terms, grad_real, grad_pred = R.terms_and_grads(_framework, real, pred, m, dtype=dtype)
    for k in R.NAMES:
        assert torch.isnan(ref[k]) and torch.isnan(terms[k]), k   # the reference's mean of an empty selection
    for g in grad_real + grad_pred:
        assert g is not None and (g == 0).all()


def test_a_plan_stands_for_its_mask():
    from waldo_amd import supervision as S
    from waldo_amd.modules.transform import ClipPlan
    from waldo_amd.nets.flp import FlpPlan
    shape = SHAPES[1]
    real, pred = R.inputs(*shape)
    b, t, no = shape[:3]
    first = FlpPlan.first_frames(b, t, 2, no + 1)
    want = S.pose_terms(real, pred, (torch.arange(t) < 2).expand(b, t), fused=False)
    m = R.mask("holes", b, t)
    for plan, ref in ((first, want), (first.frames, want), (FlpPlan.from_mask(m, no + 1), _framework(real, pred, m)),
                      (ClipPlan.from_mask(m, no + 1), _framework(real, pred, m))):
        got = S.pose_terms(real, pred, plan, fused=False)
        for k in R.NAMES:
            assert torch.equal(got[k], ref[k]), k
    frames = first.frames
    assert frames._pose_mask.dtype == torch.uint8 and frames._pose_mask.shape == (b, t)
    kept = frames._pose_mask
    S.pose_terms(real, pred, first, fused=False)
    assert frames._pose_mask is kept   # built once


def test_refusals():
    from waldo_amd import supervision as S
    real, pred = R.inputs(*SHAPES[0])
    b, t = SHAPES[0][:2]
    m = R.mask("leading", b, t)
    assert set(S.pose_terms(real, pred, m)) == set(R.NAMES) == set(S.POSE_TERMS)
    with pytest.raises(ValueError, match="3-tuples"):
        S.pose_terms(real[:2], pred[:2], m)
    with pytest.raises(ValueError, match="rec_bg_pose pair disagrees"):
        S.pose_terms(real, (pred[0], pred[1][:, :, :, :3], pred[2]), m)
    with pytest.raises(ValueError, match="rec_occ_score pair disagrees"):
        S.pose_terms(real, (pred[0], pred[1], pred[2].double()), m)
    with pytest.raises(ValueError, match=r"rec_occ_score must be a floating \(B, T, ...\)"):
        S.pose_terms(real[:2] + (real[2][:, :2],), pred[:2] + (pred[2][:, :2],), m)
    with pytest.raises(ValueError, match="rec_bg_pose must be a floating"):
        S.pose_terms((real[0], real[1].double(), real[2]), (pred[0], pred[1].double(), pred[2]), m)
    with pytest.raises(ValueError, match="boolean"):
        S.pose_terms(real, pred, m.float())
    with pytest.raises(ValueError, match="boolean"):
        S.pose_terms(real, pred, m[0])
    with pytest.raises(ValueError, match="boolean"):
        S.pose_terms(real, pred, None)
    with pytest.raises(ValueError, match="does not cover"):
        S.pose_terms(real, pred, m[:, :2])
    with pytest.raises(ValueError, match="does not cover"):
        S.pose_terms(real, pred, m.t())
    with pytest.raises(ValueError, match=r"is on meta, the poses are on cpu"):
        S.pose_terms(real, pred, m.to("meta"))
    from waldo_amd.nets.flp import FlpPlan
    with pytest.raises(ValueError, match="the plan's mask.*does not cover"):
        S.pose_terms(real, pred, FlpPlan.first_frames(b, t + 1, 1, 4))


# ---------------------------------------------------------------------------------------------------------------------
# the step driver
# ---------------------------------------------------------------------------------------------------------------------
SMALL_LVD = dict(embed_dim=32, num_heads=2, oe_depth=1, pe_depth=1, num_obj=3, obj_shape=[2, 2], latent_shape=[4, 4])
SMALL_FLP = dict(pg_com_depth=1, pg_enc_depth=1, pg_dec_depth=1, zero_init_dec=False)


def test_recipe_options():
    from waldo_amd.tools import demo
    from waldo_amd.tools.flp_step import RECIPE_WEIGHTS, flp_recipe_opt, lvd_recipe_opt
    n, f = lvd_recipe_opt(), flp_recipe_opt()
    assert RECIPE_WEIGHTS == {"rec_obj_pose": 1.0, "rec_bg_pose": 1.0, "rec_occ_score": 0.01}
    assert (n.pe_estimator_init_mode, n.oe_num_timesteps, n.use_last_pose_decoder, n.ctx_len) == ("zero", 5, True, 4)
    assert (n.input_rgb, n.input_lyt, n.input_flow, n.dim, n.aspect_ratio) == (False, True, True, 128, 2)
    assert demo.lvd_demo_opt(n).latent_shape == [8, 16]      # the raster rule holds at the recipe
    assert (f.embed_dim, f.num_heads, f.num_obj, f.latent_shape, f.obj_shape) == (512, 8, 16, [8, 16], [4, 4])
    assert (f.pg_com_depth, f.pg_enc_depth, f.pg_dec_depth, f.pg_num_timesteps) == (2, 4, 4, 14)
    assert f.use_last_pose_decoder and f.unconstrained_pose_decoder and f.zero_init_dec and f.cat_z
    assert f.bg_mul_pose_decoder == 1.2 and (f.mul_delta_obj, f.init_scale_obj, f.mul_scale_obj) == (0.2, 0.25, 0.25)


def test_a_tiny_step_on_the_cpu():
    from waldo_amd.tools import demo
    from waldo_amd.tools.flp_step import RECIPE_WEIGHTS, FlpStep
    with pytest.raises(ValueError, match="objective"):
        FlpStep(1, "cpu", objective="fused")
    with pytest.raises(ValueError, match="latent_shape"):     # the raster rule: 64 x 64 at patch 16 is 4 x 4 tokens
        FlpStep(2, "cpu", frames=6, ctx_len=4, dim=64, aspect_ratio=1, lvd_over=dict(SMALL_LVD, latent_shape=[8, 16]))
    with pytest.raises(ValueError, match="graph"):
        FlpStep(2, "cpu", graph=True, frames=6, dim=64, aspect_ratio=1, lvd_over=SMALL_LVD, flp_over=SMALL_FLP)
    step = FlpStep(2, "cpu", frames=6, ctx_len=4, dim=64, aspect_ratio=1, lvd_over=SMALL_LVD, flp_over=SMALL_FLP)
    assert demo.lvd_demo_opt(step.lvd_opt).latent_shape == [4, 4] == step.flp_opt.latent_shape
    assert (step.flp_opt.embed_dim, step.flp_opt.num_obj, step.flp_opt.obj_shape) == (32, 3, [2, 2])
    assert step.lyt.shape == (2, 6, 20, 64, 64) and step.flow.shape == (2, 6, 2, 64, 64)
    loss = step()
    assert loss.ndim == 0 and torch.isfinite(loss) and set(step.terms) == set(RECIPE_WEIGHTS)
    assert torch.allclose(loss, sum(RECIPE_WEIGHTS[k] * v.detach() for k, v in step.terms.items()), rtol=1e-6, atol=0)
    assert step.grads_finite()
    assert any(bool(p.grad.abs().max() > 0) for p in step.flp.parameters())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in step.flp.parameters())
    assert all(p.grad is None for p in step.lvd.parameters())
    # the same step again: the same loss (the gradients do not accumulate); evaluate: the same terms without a backward
    first = {k: p.grad.clone() for k, p in step.flp.named_parameters()}
    assert torch.equal(step(), loss)
    assert all(torch.equal(p.grad, first[k]) for k, p in step.flp.named_parameters())
    ev = step.evaluate()
    assert torch.equal(ev["loss"], loss) and all(torch.equal(ev[k], step.terms[k]) for k in RECIPE_WEIGHTS)
    assert not ev["loss"].requires_grad
    # per-clip context lengths: a boolean mask; against the reference's spelling on the same producer outputs
    m = torch.tensor([[True, True, False, False, False, False], [True, True, True, True, True, False]])
    masked = step(ctx_mask=m)
    assert torch.isfinite(masked) and not torch.equal(masked, loss)
    inputs = step.producers()
    with torch.no_grad():
        pred = step.flp(*inputs, ctx_mask=m)
    want = R.pose_terms(inputs[:3], pred, m)
    for k in R.NAMES:
        close(step.terms[k], want[k], rel=True, what=f"masked step {k}")
