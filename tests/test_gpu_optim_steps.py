"""GPU: the training drivers with ``optimizer=`` -- ``FlpStep`` eager against the same step replayed from ONE graph that
holds the update too, ``optimizer=None`` leaving the parameters alone, and one training step of ``LvdStep`` and ``WifStep``
with the reference networks."""
import pytest
import torch

from parity import close

pytestmark = pytest.mark.gpu
# tests/test_gpu_flp_step.py's small networks, by value
SMALL = dict(frames=6, ctx_len=4, dim=128, aspect_ratio=1,
             lvd_over=dict(embed_dim=64, num_heads=2, oe_depth=1, pe_depth=1, num_obj=3, latent_shape=[8, 8]),
             flp_over=dict(pg_com_depth=1, pg_enc_depth=1, pg_dec_depth=1, pg_num_timesteps=6, zero_init_dec=False))


def test_flp_step_trains_eagerly_and_from_one_graph(dev):
    from waldo_amd import optim
    from waldo_amd.tools.flp_step import FlpStep
    eager = FlpStep(2, dev, seed=3, optimizer="adam", **SMALL)
    assert type(eager.optimizer) is optim.Adam
    initial = {k: p.detach().clone() for k, p in eager.flp.named_parameters()}
    losses = [eager().clone() for _ in range(3)]
    graphed = FlpStep(2, dev, seed=3, graph=True, optimizer="adam", **SMALL)
    # the capture's warm-up steps left the parameters and the optimizer's state as they were
    for k, p in graphed.flp.named_parameters():
        assert torch.equal(p.detach(), initial[k]), k
    assert float(graphed.optimizer.step_count) == 0 and float(graphed.optimizer.skipped) == 0
    assert all(not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()) for st in graphed.optimizer.state.values())
    replayed = [graphed().clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(replayed[0], losses[0])                                # the eager bits
    assert not torch.equal(losses[2], losses[0]) and not torch.equal(replayed[2], replayed[0])   # the weights moved
    moved = 0
    for k, p in graphed.flp.named_parameters():
        want = dict(eager.flp.named_parameters())[k].detach() - initial[k]
        close(p.detach() - initial[k], want, rel=True, what=f"replayed update {k}")   # (as the replay test's gradients)
        moved += int(bool(want.abs().max() > 0))
    assert moved > 0
    for s in (eager, graphed):
        assert float(s.optimizer.step_count) == 3 and float(s.optimizer.skipped) == 0
        assert torch.isfinite(s.optimizer.grad_norm) and float(s.optimizer.grad_norm) > 0


def test_flp_step_without_an_optimizer_leaves_the_parameters(dev):
    from waldo_amd.tools.flp_step import FlpStep
    s = FlpStep(2, dev, seed=3, **SMALL)
    assert s.optimizer is None
    initial = [p.detach().clone() for p in s.flp.parameters()]
    first = s().clone()
    second = s().clone()
    assert torch.equal(first, second)
    assert all(torch.equal(p.detach(), p0) for p, p0 in zip(s.flp.parameters(), initial))
    with pytest.raises(ValueError, match="optimizer must be"):
        FlpStep(2, dev, seed=3, optimizer="sgd", **SMALL)


def _one_training_step(step, net):
    initial = [p.detach().clone() for p in net.parameters()]
    loss = step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    opt = step.optimizer
    assert float(opt.step_count) == 1 and float(opt.skipped) == 0
    changed = 0
    for p, p0 in zip(net.parameters(), initial):
        if p.grad is None or not bool(p.grad.abs().max() > 0):
            assert torch.equal(p.detach(), p0)          # no gradient: left alone
        else:
            changed += int(not torch.equal(p.detach(), p0))
    assert changed > 0


def test_lvd_step_trains_the_reference_networks(dev):
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(1, dev, seed=1, nets="reference", optimizer="adam")
    _one_training_step(step, step.net)


def test_wif_step_trains_the_reference_unet(dev):
    """(The smallest step the driver takes: frames at the layers' 128 x 256, a UNet 16 wide with two levels.  At the
    recipe's 512 x 1024 the convolution library spends ~30 s choosing kernels at the first call on a fresh machine.)"""
    from waldo_amd import optim
    from waldo_amd.tools.wif_step import WifStep
    step = WifStep(1, dev, unet="reference", optimizer="adam", opt_over=dict(ii_embed_dim=16, ii_depth=2, load_dim=128))
    assert type(step.optimizer) is optim.Adam
    _one_training_step(step, step.unet)
