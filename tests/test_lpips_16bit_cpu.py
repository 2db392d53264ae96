"""CPU: the 16-bit side of LPIPS off the kernel route -- ``WF.lpips_level`` on bf16 / fp16 maps with an fp32 ``w`` (what
autocast produces) is the chain on the maps widened to fp32, its output fp32 and its gradients of the maps' type; the
route of same-type 16-bit operands is unchanged; ``LPIPS.act_dtype`` and ``WifStep(lpips_dtype=)`` check their
arguments before the device."""
import pytest
import torch

import lpips_ref as R
from parity import close
from test_gpu_unet_16bit import close16   # (the bound of a result stored in 16 bits: that module's docstring)

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("trainable_w", [False, True])
@pytest.mark.parametrize("T", DTYPES, ids=["bf16", "fp16"])
def test_the_mixed_route_is_the_chain_on_the_widened_maps(T, trainable_w):
    from waldo_amd import functional as WF
    f0, f1, w = R.features((3, 5, 7, 9), 1)
    f0, f1 = f0.to(T).requires_grad_(), f1.to(T).requires_grad_()
    w4 = w.view(1, -1, 1, 1).clone().requires_grad_(trainable_w)
    got = WF.lpips_level(f0, f1, w4)
    assert got.shape == (3,) and got.dtype == torch.float32
    g0, g1 = torch.autograd.grad(got.sum(), (f0, f1), retain_graph=trainable_w)
    assert g0.dtype == T and g1.dtype == T and g0.shape == f0.shape

    def chain(dt):
        x0, x1 = (t.detach().to(dt).requires_grad_() for t in (f0, f1))
        xw = w.to(dt).requires_grad_()
        out = R.level(x0, x1, xw)
        return (out.detach(),) + torch.autograd.grad(out.sum(), (x0, x1, xw))

    same, exact = chain(torch.float32), chain(torch.float64)
    close(got, same[0], rel=True, exact=exact[0], what=f"cpu mixed {T} out")
    for i, g in ((1, g0), (2, g1)):   # the fp32 gradient rounded once to T by the widening's backward
        close16(g, same[i], exact[i], T, rel=True, what=f"cpu mixed {T} grad_f{i - 1}")
    if trainable_w:
        gw, = torch.autograd.grad(got.sum(), w4)
        assert gw.dtype == torch.float32
        close(gw.reshape(-1), same[3], rel=True, exact=exact[3], what=f"cpu mixed {T} grad_w")
    assert torch.equal(WF.lpips_level(f0, f0.detach().clone(), w), torch.zeros(3))


@pytest.mark.parametrize("T", DTYPES, ids=["bf16", "fp16"])
def test_same_type_16_bit_operands_keep_their_route_and_type(T):
    """16-bit maps with a ``w`` of the SAME type still are ``lpips_level_framework`` in that type, bit for bit."""
    from waldo_amd import functional as WF
    f0, f1, w = R.features((3, 5, 7, 9), 2, dtype=T)
    got = WF.lpips_level(f0, f1, w)
    assert got.dtype == T and torch.equal(got, WF.lpips_level_framework(f0, f1, w))


def test_mixed_operands_that_are_still_refused():
    from waldo_amd import functional as WF
    f = torch.rand(2, 5, 3, 4)
    with pytest.raises(ValueError, match="C = 5"):          # fp32 maps with a 16-bit w: not what autocast produces
        WF.lpips_level(f, f, torch.rand(5).bfloat16())
    with pytest.raises(ValueError, match="C = 5"):
        WF.lpips_level(f.bfloat16(), f.bfloat16(), torch.rand(5).half())
    with pytest.raises(ValueError, match="C = 5"):
        WF.lpips_level(f.half(), f.half(), torch.rand(5).double())
    with pytest.raises(ValueError, match="C = 5"):
        WF.lpips_level(f.half(), f.half(), torch.rand(4))
    with pytest.raises(ValueError, match="disagree"):
        WF.lpips_level(f.half(), f.bfloat16(), torch.rand(5))


def test_act_dtype_arguments():
    from waldo_amd.nets import LPIPS
    from waldo_amd.tools.evaluate import LPIPS_DTYPES
    for bad in (torch.float64, "bf16", torch.float32, torch.int8):
        with pytest.raises(ValueError, match="act_dtype"):
            LPIPS("alex", act_dtype=bad)
    torch.manual_seed(3)
    m = LPIPS("alex")
    assert m.act_dtype is None
    for T in DTYPES:
        loaded = LPIPS.load("alex", state=m.state_dict(), act_dtype=T)
        assert loaded.act_dtype == T and loaded.fused
        assert all(p.dtype == torch.float32 for p in loaded.parameters())   # the parameters stay fp32: autocast casts
    assert LPIPS_DTYPES == {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def test_act_dtype_module_on_the_cpu_gives_fp32():
    """bf16 activations on the CPU (the framework route of the mixed ``lpips_level``): an fp32 (N, 1, 1, 1) and an fp32
    input gradient; fused and ``fused=False`` agree bit for bit there (both are the chain on the widened taps)."""
    from waldo_amd.nets import LPIPS
    torch.manual_seed(4)
    m = LPIPS("alex", chunk=2)
    g = torch.Generator().manual_seed(6)
    in0 = (torch.rand(3, 3, 95, 127, generator=g) * 2 - 1).requires_grad_()
    in1 = (in0.detach() + 0.2 * torch.randn(3, 3, 95, 127, generator=g)).clamp(-1, 1)
    want = m(in0, in1).detach()
    outs = []
    for fused in (True, False):
        m16 = LPIPS.load("alex", state=m.state_dict(), chunk=2, fused=fused, act_dtype=torch.bfloat16)
        out = m16(in0, in1)
        grad, = torch.autograd.grad(out.sum(), in0)
        assert out.shape == (3, 1, 1, 1) and out.dtype == torch.float32
        assert grad.dtype == torch.float32 and torch.isfinite(grad).all() and grad.abs().max() > 0
        assert torch.isfinite(out).all() and (out > 0).all()
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], want)   # (the taps were rounded: not the fp32 module's bits)


def test_wif_step_lpips_dtype_arguments():
    from waldo_amd.nets import LPIPS
    from waldo_amd.tools.wif_step import WifStep
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="lpips_dtype"):
        WifStep(1, dev, objective="sharp", lpips_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="lpips_dtype"):
        WifStep(1, dev, lpips_dtype=torch.float16)
    torch.manual_seed(5)
    with pytest.raises(ValueError, match="disagrees"):
        WifStep(1, dev, objective="recipe", lpips=LPIPS("vgg"), lpips_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="disagrees"):
        WifStep(1, dev, objective="recipe", lpips=LPIPS("vgg", act_dtype=torch.float16), lpips_dtype=torch.bfloat16)
