"""GPU: the ``LPIPS`` module (fused levels against framework levels against the fp64 restatement of tests/lpips_ref.py),
the ``"lpips"`` entry of ``frame_metrics`` and the recipe objective of ``WifStep``.

The convolution library does not repeat its bits from call to call at these shapes: two runs of the SAME framework-only
module differed by up to 4.5e-4 of the input gradient's scale (alex, the backward) and in the last bits of a forward,
whichever of the two modules ran first.  So the comparison of the two MODULES runs both on the framework's own
convolutions (``cudnn.flags(enabled=False)``: what is compared is the levels and their place in the graph, the backbone
is the same arithmetic on both sides), as does the bit-for-bit comparison of the ``WifStep`` objectives.  The shipped
route -- the library's convolutions feeding the fused levels and taking their gradients back -- has a test of its own
that shares ONE pass through the library between the two sides
(``test_fused_levels_on_the_librarys_convolutions``)."""
import functools

import pytest
import torch

import lpips_ref as R
from parity import close

pytestmark = pytest.mark.gpu
IMAGES = {"vgg": (3, 3, 40, 56), "alex": (3, 3, 95, 127)}   # alex: odd taps (23 x 31, 11 x 15, 5 x 7)


@functools.lru_cache(maxsize=None)
def module(net):
    from waldo_amd.nets import LPIPS
    return LPIPS(net, chunk=2, generator=torch.Generator().manual_seed(17))   # (three images: chunks of two and one)


@functools.lru_cache(maxsize=None)
def case(net):
    """A pair of image batches, a weight per image, and the restatement's value and gradient in fp64 on the CPU."""
    g = torch.Generator().manual_seed(23)
    shape = IMAGES[net]
    in0 = torch.rand(*shape, generator=g) * 2 - 1
    in1 = (in0 + 0.2 * torch.randn(*shape, generator=g)).clamp(-1, 1)
    weight = torch.rand(shape[0], 1, 1, 1, generator=g) + 0.5
    state = {k: v.double() for k, v in module(net).state_dict().items()}   # (the cached module stays on the CPU)
    x = in0.double().requires_grad_()
    out = R.lpips(net, state, x, in1.double())
    grad, = torch.autograd.grad((out * weight.double()).sum(), x)
    return in0, in1, weight, out.detach(), grad


def run(m, in0, in1, weight, dev):
    x = in0.to(dev).requires_grad_()
    out = m(x, in1.to(dev))
    grad, = torch.autograd.grad((out * weight.to(dev)).sum(), x)
    return out.detach(), grad


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_fused_levels_equal_framework_levels_and_the_restatement(dev, net):
    from waldo_amd import _lib
    from waldo_amd.nets import LPIPS
    in0, in1, weight, out64, grad64 = case(net)
    state = module(net).state_dict()
    fused = LPIPS.load(net, state=state, chunk=2).to(dev)
    plain = LPIPS.load(net, state=state, chunk=2, fused=False).to(dev)
    with torch.backends.cudnn.flags(enabled=False):   # (see the module docstring)
        ref_out, ref_grad = run(plain, in0, in1, weight, dev)
        with _lib.KernelTimer() as timer:
            out, grad = run(fused, in0, in1, weight, dev)
        torch.cuda.synchronize()
    calls = {k: len(v) for k, v in timer.pairs.items() if "lpips" in k}
    assert calls == {"waldo_lpips_level_fwd": 10, "waldo_lpips_level_bwd": 10}, calls   # five levels x two chunks
    assert out.shape == (3, 1, 1, 1) and out.dtype == torch.float32
    close(out, ref_out, rel=True, exact=out64, what=f"{net} value")
    close(grad, ref_grad, rel=True, exact=grad64, what=f"{net} grad in0")
    whole = LPIPS.load(net, state=state, chunk=8).to(dev)
    close(whole(in0.to(dev), in1.to(dev)), out, rel=True, what=f"{net} chunk 8 against chunk 2")


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_fused_levels_on_the_librarys_convolutions(dev, net):
    """The shipped route: the taps come out of the library's convolutions (in-place ReLUs and all) and the levels'
    gradients go back through them.  One forward through the backbone serves both sides, so the library's own
    run-to-run differences cancel: the fused and the framework levels are compared on the SAME taps -- value and the
    gradient at every tap, against the chain in fp64 on those taps -- and the gradient with respect to ``in0`` by the
    backbone's linearity: the backward of (fused - framework) tap gradients is their difference at ``in0``, and is held
    to the bound at the scale of the whole gradient (a relative error of the library's acts on the difference only)."""
    from waldo_amd import functional as WF
    from waldo_amd.nets import LPIPS
    in0, in1, weight, out64, grad64 = case(net)
    m = LPIPS.load(net, state=module(net).state_dict()).to(dev)
    x = in0.to(dev).requires_grad_()
    a, b = m.scaling_layer(x), m.scaling_layer(in1.to(dev))
    taps = []
    for k in range(5):
        piece = getattr(m.net, f"slice{k + 1}")
        a, b = piece(a), piece(b)
        taps.append((a, b))
    wt = weight.to(dev).view(-1)
    with torch.no_grad():
        fused = sum(WF.lpips_level(a, b, m.lin(k)) for k, (a, b) in enumerate(taps))
        plain = sum(WF.lpips_level_framework(a, b, m.lin(k)) for k, (a, b) in enumerate(taps))
    close(fused, plain, rel=True, exact=out64.view(-1), what=f"{net} library route value")
    g_fused, g_plain = [], []
    for k, (a, b) in enumerate(taps):   # the level's own gradient at its tap, on the tap as the library left it
        for level, keep in ((WF.lpips_level, g_fused), (WF.lpips_level_framework, g_plain)):
            leaf = a.detach().requires_grad_()
            keep.append(torch.autograd.grad((level(leaf, b, m.lin(k)) * wt).sum(), leaf)[0])
        a64 = a.detach().double().cpu().requires_grad_()
        d64 = R.level(a64, b.detach().double().cpu(), m.lin(k).double().cpu())
        want, = torch.autograd.grad((d64 * weight.double().view(-1)).sum(), a64)
        close(g_fused[k], g_plain[k], rel=True, exact=want, what=f"{net} library route grad at tap {k}")
    own = [a for a, _ in taps]
    whole, = torch.autograd.grad(own, x, g_plain, retain_graph=True)
    diff, = torch.autograd.grad(own, x, [f - p for f, p in zip(g_fused, g_plain)])
    assert whole.abs().max() > 0
    close(whole + diff, whole, rel=True, what=f"{net} library route grad in0: framework levels + J^T (fused - framework)")


@functools.lru_cache(maxsize=None)
def clip():
    g = torch.Generator().manual_seed(29)
    real = torch.rand(2, 3, 3, 176, 192, generator=g) * 2.2 - 1.1        # (values beyond the span: clamped)
    pred = real + 0.15 * torch.randn(2, 3, 3, 176, 192, generator=g)
    return pred, real


def by_hand(x, quantize):
    """frame_metrics' documented quantisation of a [-1, 1] clip (or of its bytes), as frames in [-1, 1]."""
    if x.dtype == torch.uint8:
        u = x.float() / 255.0
    else:
        u = ((x + 1.0) / 2.0).clamp(0.0, 1.0)
        if quantize == "trunc":
            u = torch.trunc(u * 255.0) / 255.0
        elif quantize == "round":
            u = torch.trunc(u * 255.0 + 0.5) / 255.0
    return (2.0 * u - 1.0).flatten(0, 1)


@pytest.mark.parametrize("form,quantize", [("fp32", "trunc"), ("fp32", "none"), ("fp32", "round"), ("uint8", "trunc")])
def test_frame_metrics_lpips(dev, form, quantize):
    from waldo_amd.metrics import frame_metrics
    from waldo_amd.nets import LPIPS
    m = LPIPS.load("alex", state=module("alex").state_dict()).to(dev)
    pred, real = (t.to(dev) for t in clip())
    if form == "uint8":
        pred, real = (torch.trunc(((t + 1) / 2).clamp(0, 1) * 255).to(torch.uint8) for t in (pred, real))
    got = frame_metrics(pred, real, metrics=("lpips", "msssim"), quantize=quantize, lpips=m)
    assert list(got) == ["lpips", "msssim"]
    assert got["lpips"].shape == (2, 3) and got["lpips"].dtype == torch.float32 and (got["lpips"] > 0).all()
    with torch.no_grad():
        want = m(by_hand(pred, quantize), by_hand(real, quantize)).view(2, 3)
    close(got["lpips"], want, rel=True, what=f"lpips metric {form} {quantize}")
    alone = frame_metrics(pred, real, metrics=("msssim",), quantize=quantize)
    assert torch.equal(got["msssim"], alone["msssim"])                   # the other metrics are what they were
    close(frame_metrics(pred, real, metrics=("lpips",), quantize=quantize, lpips=m)["lpips"], got["lpips"], rel=True,
          what=f"lpips metric {form} {quantize}: asked for alone")
    if form == "uint8":   # the bytes are the fp32 clip's "trunc" bytes: the same frames either way
        f32 = frame_metrics(*(t.to(dev) for t in clip()), metrics=("lpips",), quantize="trunc", lpips=m)["lpips"]
        close(f32, got["lpips"], rel=True, what="lpips metric: bytes against the fp32 clip")


def test_wif_step_recipe_objective(dev):
    from waldo_amd.tools.wif_step import WifStep
    step = WifStep(1, dev, objective="recipe")
    loss = step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and step.grads_finite()
    assert set(step.terms) == {"sharp_vid", "lpips_vid"}
    assert all(t.ndim == 0 and not t.requires_grad for t in step.terms.values()) and step.terms["lpips_vid"] > 0
    assert torch.equal(loss.detach(), step.terms["sharp_vid"] + step.terms["lpips_vid"])
    assert step.lpips.net_name == "vgg" and step.lpips.fused


def test_wif_step_sharp_objective_has_the_parents_bits(dev):
    """``objective="sharp"`` is the parent's step bit for bit: the default step, the step asked for by name, the parent's
    expression written out on the step's own tensors give ONE loss, and the two steps the same gradients.  On the framework's own convolutions (see the module docstring): the stand-in network is a
    convolution, and two passes through the library need not repeat their bits."""
    from waldo_amd.tools.wif_step import WifStep
    with torch.backends.cudnn.flags(enabled=False):
        default, sharp = WifStep(1, dev), WifStep(1, dev, objective="sharp")
        a, b = default(), sharp()
        with torch.no_grad():   # the parent's lines (wif_step.py: inp_output, real, loss), on the default step's tensors
            inp_output = default.wif(default.raw_output)
            real = default.vid[:, default.ctx_len:]
            want = (inp_output[:, :, :3] - real).abs().mean()
        torch.cuda.synchronize()
    assert default.objective == "sharp" and set(sharp.terms) == set(default.terms) == {"sharp_vid"} and sharp.lpips is None
    assert torch.equal(a.detach(), b.detach()), (a.item(), b.item())
    assert torch.equal(a.detach(), want), (a.item(), want.item())
    for p, q in zip(default.unet.parameters(), sharp.unet.parameters()):
        assert p.grad is not None and p.grad.abs().max() > 0 and torch.equal(p.grad, q.grad)
