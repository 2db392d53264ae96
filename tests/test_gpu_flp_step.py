"""GPU: ``tools.flp_step.FlpStep`` with small networks (64 wide, 2 heads, depth 1, 6 frames of 128 x 128, 4 context
frames, noise options off): a step that reads nothing on the host, the kernel objective against the framework one on
the same producer outputs, the step replayed from one graph, and a boolean mask with per-clip context lengths."""
import copy

import pytest
import torch

import pose_terms_ref as R
from parity import close

pytestmark = pytest.mark.gpu
SMALL = dict(frames=6, ctx_len=4, dim=128, aspect_ratio=1,
             lvd_over=dict(embed_dim=64, num_heads=2, oe_depth=1, pe_depth=1, num_obj=3, latent_shape=[8, 8]),
             flp_over=dict(pg_com_depth=1, pg_enc_depth=1, pg_dec_depth=1, pg_num_timesteps=6, zero_init_dec=False))


@pytest.fixture(scope="module")
def step(dev):
    from waldo_amd.tools.flp_step import FlpStep
    s = FlpStep(2, dev, seed=3, **SMALL)
    s()   # (the libraries' first calls and the cached index tensors are behind it)
    return s


def test_a_step_reads_nothing_on_the_host(step):
    from waldo_amd import _lib
    from waldo_amd.tools.flp_step import RECIPE_WEIGHTS
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with _lib.KernelTimer() as timer:
            loss = step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    calls = {k: len(v) for k, v in timer.pairs.items()}
    assert calls.get("waldo_pose_l1_fwd") == 1 and calls.get("waldo_pose_l1_bwd") == 1, calls
    assert calls.get("waldo_token_attention_clips_fwd") == 3, calls   # the encoder's block, the decoder's two
    assert torch.isfinite(loss) and step.grads_finite()
    assert torch.allclose(loss, sum(RECIPE_WEIGHTS[k] * v.detach() for k, v in step.terms.items()), rtol=1e-6, atol=0)
    assert all(p.grad is None for p in step.lvd.parameters())
    assert any(bool(p.grad.abs().max() > 0) for p in step.flp.parameters())
    ev = step.evaluate()
    assert torch.equal(ev["loss"], loss) and not ev["loss"].requires_grad


def _loss_and_grads(flp, inputs, ctx_mask, objective):
    from waldo_amd.tools.flp_step import RECIPE_WEIGHTS
    flp.zero_grad(set_to_none=True)
    terms = objective(inputs[:3], flp(*inputs, ctx_mask=ctx_mask), ctx_mask)
    loss = sum(RECIPE_WEIGHTS[k] * terms[k] for k in R.NAMES)
    loss.backward()
    return loss.detach(), {k: p.grad.clone() for k, p in flp.named_parameters()}


@pytest.fixture(scope="module")
def exact(step):
    """The step's loss and parameter gradients from its producer outputs in fp64 on the CPU: ``FLP(fused=False)`` and the
    reference's spelling of the objective."""
    inputs = tuple(x.detach().cpu().double() for x in step.producers())
    flp = copy.deepcopy(step.flp).cpu().double()
    flp.fused = False
    m = (torch.arange(step.frames) < step.ctx_len).expand(step.clips, step.frames)
    return _loss_and_grads(flp, inputs, m, R.pose_terms)


@pytest.mark.parametrize("route", ["framework", "kernel"])
def test_kernel_and_framework_objectives_agree_on_parameter_gradients(step, exact, route):
    from waldo_amd import functional as WF
    from waldo_amd import supervision as S
    inputs = step.producers()
    with WF.token_attention_backward_route(route):
        got = _loss_and_grads(step.flp, inputs, step.plan, lambda r, p, m: S.pose_terms(r, p, m, fused=True))
        ref = _loss_and_grads(step.flp, inputs, step.plan, lambda r, p, m: S.pose_terms(r, p, m, fused=False))
    close(got[0], ref[0], rel=True, exact=exact[0], what=f"{route} loss")
    for k in exact[1]:
        close(got[1][k], ref[1][k], rel=True, exact=exact[1][k], what=f"{route} grad {k}")


def test_the_step_replays_from_one_graph(step):
    from waldo_amd.tools.flp_step import FlpStep
    loss = step().clone()
    terms = {k: v.detach().clone() for k, v in step.terms.items()}
    grads = {k: p.grad.clone() for k, p in step.flp.named_parameters()}
    graphed = FlpStep(2, step.device, seed=3, graph=True, **SMALL)
    with pytest.raises(ValueError, match="eagerly"):
        graphed(ctx_mask=torch.zeros(2, 6, dtype=torch.bool, device=step.device))
    first = graphed().clone()
    assert torch.equal(first, loss)                                          # the eager bits
    for k in terms:
        assert torch.equal(graphed.terms[k].detach(), terms[k]), k
    for k, p in graphed.flp.named_parameters():
        close(p.grad, grads[k], rel=True, what=f"replayed grad {k}")        # (index_select's backward may use atomics)
    assert graphed.grads_finite()
    kept = graphed.flow.clone()
    graphed.flow.zero_()                                                      # new data in the static clip: a new step
    other = graphed().clone()
    graphed.flow.copy_(kept)
    again = graphed().clone()
    torch.cuda.synchronize()
    assert not torch.equal(other, loss) and torch.equal(again, loss)


def test_a_boolean_mask_with_per_clip_context_lengths(step):
    m = torch.tensor([[True, True, False, False, False, False], [True, True, True, True, True, False]], device=step.device)
    loss = step(ctx_mask=m)
    assert torch.isfinite(loss) and step.grads_finite()
    inputs = step.producers()
    with torch.no_grad():
        pred = step.flp(*inputs, ctx_mask=m)
    want32 = R.pose_terms(inputs[:3], pred, m)
    want64 = R.pose_terms([x.cpu().double() for x in inputs[:3]], [x.cpu().double() for x in pred], m.cpu())
    for k in R.NAMES:
        close(step.terms[k], want32[k], rel=True, exact=want64[k], what=f"masked step {k}")
