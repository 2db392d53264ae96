"""GPU: ``LPIPS(net, act_dtype=T)`` -- the backbone under autocast, every 16-bit tap through the 16-bit level kernels
(waldo_lpips_level_fwd_dt / _bwd_dt) -- with the ``"lpips"`` entry of ``frame_metrics`` and ``WifStep(lpips_dtype=)``.

The images, the chunking and the seeded random-weight module are tests/test_gpu_lpips.py's (vgg 3 x 3 x 40 x 56; alex
3 x 3 x 95 x 127, whose taps are odd: 23 x 31, 11 x 15, 5 x 7).

Same taps (the method of ``test_fused_levels_on_the_librarys_convolutions``): ONE pass through the backbone under
autocast serves both sides, so the library's run-to-run differences cancel.  At every tap the kernel's value and tap
gradient are compared with the chain on the WIDENED tap in fp32 on the device and in fp64 on the CPU, under the bounds
of tests/test_gpu_lpips_level_16bit.py (the value: ``parity.close``; the gradient in T: ``close16``).

Whole module: the fused module and the same module with ``fused=False`` (the chain on the widened taps) both round at
the same points -- the 16-bit taps on the way up, the 16-bit tap gradients on the way down -- so their distances from
the fp64 restatement are draws of the same rounding noise: the fused route's rms distance may be at most twice the
framework route's own, for the value and for the ``in0`` gradient (the rule of tests/test_gpu_unet_16bit.py)."""
import pytest
import torch

import lpips_ref as R
from parity import close
from test_gpu_lpips import case, clip, module
from test_gpu_unet_16bit import close16, two_x_rule

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def ids(t):
    return str(t).replace("torch.", "")


def lpips_calls(timer):
    return {k: len(v) for k, v in timer.pairs.items() if "lpips" in k}


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_the_kernels_on_the_taps_of_the_backbone_under_autocast(dev, net, T):
    from waldo_amd import functional as WF
    from waldo_amd.nets import LPIPS
    in0, in1, weight, _, _ = case(net)
    m = LPIPS.load(net, state=module(net).state_dict(), act_dtype=T).to(dev)
    with torch.no_grad():
        a, b = m.scaling_layer(in0.to(dev)), m.scaling_layer(in1.to(dev))
        taps = []
        for k in range(5):
            piece = getattr(m.net, f"slice{k + 1}")
            with torch.autocast("cuda", dtype=T):
                a, b = piece(a), piece(b)
            taps.append((a, b))   # (every slice begins with a pool or a convolution: nothing writes into a tap)
    wt = weight.to(dev).view(-1)
    for k, (a, b) in enumerate(taps):
        assert a.dtype == T and b.dtype == T
        lin = m.lin(k)
        leaf = a.detach().requires_grad_()
        out = WF.lpips_level(leaf, b, lin)
        grad, = torch.autograd.grad(out, leaf, wt)
        assert out.dtype == torch.float32 and grad.dtype == T
        refs = []
        for device, dt in (("cuda:0", torch.float32), ("cpu", torch.float64)):
            x = a.detach().to(device=device, dtype=dt).requires_grad_()
            d = R.level(x, b.detach().to(device=device, dtype=dt), lin.detach().to(device=device, dtype=dt))
            g, = torch.autograd.grad(d, x, wt.to(device=device, dtype=dt))
            refs.append((d.detach().cpu(), g.cpu()))
        close(out.detach(), refs[0][0], rel=True, exact=refs[1][0], what=f"{net} {T} tap {k} value")
        close16(grad, refs[0][1], refs[1][1], T, rel=True, what=f"{net} {T} tap {k} grad")


def run(m, in0, in1, weight, dev):
    x = in0.to(dev).requires_grad_()
    out = m(x, in1.to(dev))
    grad, = torch.autograd.grad((out * weight.to(dev)).sum(), x)
    return out, grad


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_fused_against_the_framework_levels_under_the_same_autocast(dev, net, T):
    from waldo_amd import _lib
    from waldo_amd.nets import LPIPS
    in0, in1, weight, out64, grad64 = case(net)
    state = module(net).state_dict()
    fused = LPIPS.load(net, state=state, chunk=2, act_dtype=T).to(dev)
    plain = LPIPS.load(net, state=state, chunk=2, fused=False, act_dtype=T).to(dev)
    with _lib.KernelTimer() as timer:
        p_out, p_grad = run(plain, in0, in1, weight, dev)
        torch.cuda.synchronize()
        assert lpips_calls(timer) == {}
        out, grad = run(fused, in0, in1, weight, dev)
        torch.cuda.synchronize()
    # five levels x two chunks, and no fp32 LPIPS kernel
    assert lpips_calls(timer) == {"waldo_lpips_level_fwd_dt": 10, "waldo_lpips_level_bwd_dt": 10}, lpips_calls(timer)
    for o, g in ((out, grad), (p_out, p_grad)):
        assert o.shape == (3, 1, 1, 1) and o.dtype == torch.float32 and not o.detach().requires_grad
        assert g.dtype == torch.float32 and g.shape == in0.shape and torch.isfinite(g).all() and g.abs().max() > 0
    two_x_rule({"value": out.detach().cpu(), "grad_in0": grad.cpu()}, {"value": p_out.detach().cpu(), "grad_in0": p_grad.cpu()},
               {"value": out64, "grad_in0": grad64}, f"LPIPS {net} {T}")


def test_act_dtype_none_is_the_fp32_module(dev):
    """``act_dtype=None`` calls the fp32 kernels only, as before."""
    from waldo_amd import _lib
    from waldo_amd.nets import LPIPS
    in0, in1, weight, _, _ = case("alex")
    m = LPIPS.load("alex", state=module("alex").state_dict(), chunk=2, act_dtype=None).to(dev)
    with _lib.KernelTimer() as timer:
        run(m, in0, in1, weight, dev)
        torch.cuda.synchronize()
    assert lpips_calls(timer) == {"waldo_lpips_level_fwd": 10, "waldo_lpips_level_bwd": 10}


@pytest.mark.parametrize("T", DTYPES, ids=ids)
def test_frame_metrics_takes_the_16_bit_module(dev, T):
    from waldo_amd.metrics import frame_metrics
    from waldo_amd.nets import LPIPS
    state = module("alex").state_dict()
    m = LPIPS.load("alex", state=state, act_dtype=T).to(dev)
    pred, real = (t.to(dev) for t in clip())
    got = frame_metrics(pred, real, metrics=("lpips",), lpips=m)["lpips"]
    assert got.shape == (2, 3) and got.dtype == torch.float32 and torch.isfinite(got).all() and (got > 0).all()


def test_wif_step_lpips_dtype(dev):
    from waldo_amd import _lib
    from waldo_amd.tools.wif_step import WifStep
    step = WifStep(1, dev, objective="recipe", lpips_dtype=torch.bfloat16)
    assert step.lpips.act_dtype == torch.bfloat16 and step.lpips.net_name == "vgg" and step.lpips.fused
    with _lib.KernelTimer() as timer:
        loss = step()
        torch.cuda.synchronize()
    assert torch.isfinite(loss) and step.grads_finite() and loss.dtype == torch.float32
    assert set(step.terms) == {"sharp_vid", "lpips_vid"}
    assert torch.isfinite(step.terms["lpips_vid"]) and step.terms["lpips_vid"] > 0
    calls = lpips_calls(timer)
    assert set(calls) == {"waldo_lpips_level_fwd_dt", "waldo_lpips_level_bwd_dt"} and calls["waldo_lpips_level_fwd_dt"] == 5, calls
    plain = WifStep(1, dev, objective="recipe")
    assert plain.lpips.act_dtype is None
    with _lib.KernelTimer() as timer:
        loss32 = plain()
        torch.cuda.synchronize()
    calls = lpips_calls(timer)
    assert set(calls) == {"waldo_lpips_level_fwd", "waldo_lpips_level_bwd"}, calls   # no _dt call without the argument
    assert torch.isfinite(loss32)
