"""GPU: ``WF.lpips_level`` through its kernels (include/waldo_hip.h "LPIPS level distance") against the chain
(tests/lpips_ref.py) on the same inputs, in fp32 on the device and in fp64 on the CPU, under ``parity.close``.

The shapes (N, C, H, W): one element; odd everything; 64 channels over 39 tiles of 64 pixels with a ragged tail; channel
counts that are no multiple of the four waves or of the backward's 64-channel chunk (65, 130, 512); the five VGG taps of
a 32 x 48 frame; three of 2 x 131 072 pixels and more (thousands of workgroups per image; P a multiple of the tile, a
multiple of 4 only, odd); and 4200 channels, more than the 64 chunks of 64 that the backward's
workgroups cover side by side.  Each with
independent operands and with f1 = f0 (1 + 1e-2 randn): nearly equal maps, where an expanded form would cancel."""
import functools

import pytest
import torch

import lpips_ref as R
from parity import close

pytestmark = pytest.mark.gpu
VGG_TAPS = [(2, 64, 32, 48), (2, 128, 16, 24), (2, 256, 8, 12), (2, 512, 4, 6), (2, 512, 2, 3)]
LARGE = [(2, 3, 256, 512), (2, 6, 258, 510), (2, 5, 257, 511)]
STRIDED = [(1, 4200, 1, 5)]   # more than 64 chunks of 64 channels: the backward's workgroups stride over the chunks
SHAPES = ([(1, 1, 1, 1), (3, 5, 7, 9), (2, 64, 37, 67), (2, 65, 9, 33), (2, 130, 5, 67), (2, 512, 3, 5)] + VGG_TAPS + LARGE
          + STRIDED)
KINDS = ("independent", "near")


def chain(f0, f1, w, grad_out, device, dtype, both=False):
    """(out, grad_f0[, grad_f1]) of the chain on ``device`` in ``dtype``, back on the CPU."""
    x0 = f0.to(device=device, dtype=dtype).requires_grad_()
    x1 = f1.to(device=device, dtype=dtype).requires_grad_(both)
    out = R.level(x0, x1, w.to(device=device, dtype=dtype))
    grads = torch.autograd.grad(out, (x0, x1) if both else (x0,), grad_out.to(device=device, dtype=dtype))
    return (out.detach().cpu(),) + tuple(g.cpu() for g in grads)


def kernel(f0, f1, w, grad_out, dev, both=False):
    from waldo_amd import functional as WF
    x0 = f0.to(dev).requires_grad_()
    x1 = f1.to(dev).requires_grad_(both)
    out = WF.lpips_level(x0, x1, w.to(dev))
    grads = torch.autograd.grad(out, (x0, x1) if both else (x0,), grad_out.to(dev))
    return (out.detach(),) + grads


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """The operands, a random grad_out per image, and the chain in fp32 on the device and fp64 on the CPU: once."""
    f0, f1, w = R.features(shape, seed=sum(shape), near=1e-2 if kind == "near" else None)
    grad_out = torch.randn(shape[0], generator=torch.Generator().manual_seed(7)) + 2.0
    ref32 = chain(f0, f1, w, grad_out, "cuda:0", torch.float32)
    ref64 = chain(f0, f1, w, grad_out, "cpu", torch.float64)
    return f0, f1, w, grad_out, ref32, ref64


def compare(got, ref32, ref64, what):
    for i, name in enumerate(("out", "grad_f0", "grad_f1")[:len(got)]):
        close(got[i], ref32[i], rel=True, exact=ref64[i], what=f"{what} {name}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_chain(dev, shape, kind):
    f0, f1, w, grad_out, ref32, ref64 = reference(shape, kind)
    got = kernel(f0, f1, w, grad_out, dev)
    assert got[0].shape == (shape[0],) and got[0].dtype == torch.float32
    compare(got, ref32, ref64, f"{shape} {kind}")


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 32, 48), (2, 3, 256, 512)], ids=lambda s: "x".join(map(str, s)))
def test_storage_one_float_past_a_16_byte_boundary(dev, shape):
    """Slices of larger buffers whose first element sits 4 bytes past a 16-byte boundary: nothing may assume more than
    4-byte alignment, whatever P is."""
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, ref32, ref64 = reference(shape, "independent")
    n = f0.numel()

    def shifted(t):
        buf = torch.empty(n + 8, dtype=torch.float32, device=dev)
        start = 1 + (4 - (buf.data_ptr() // 4) % 4) % 4          # element index whose address is 16 k + 4
        view = buf[start:start + n].view(t.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view.copy_(t)

    x0, x1 = shifted(f0).requires_grad_(), shifted(f1)
    out = WF.lpips_level(x0, x1, w.to(dev))
    grad, = torch.autograd.grad(out, x0, grad_out.to(dev))
    compare((out.detach(), grad), ref32, ref64, f"{shape} shifted")


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 32, 48)], ids=lambda s: "x".join(map(str, s)))
def test_non_contiguous_operands_are_their_contiguous_copies(dev, shape):
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, _, _ = reference(shape, "independent")
    want = kernel(f0, f1, w, grad_out, dev)
    x0 = f0.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_()   # channels last
    x1 = torch.stack([f1, f1 + 1], dim=-1).to(dev)[..., 0]                                   # every second element
    assert not x0.is_contiguous() and not x1.is_contiguous()
    out = WF.lpips_level(x0, x1, w.to(dev).view(1, -1, 1, 1))
    grad, = torch.autograd.grad(out, x0, grad_out.to(dev))
    assert torch.equal(out, want[0]) and torch.equal(grad, want[1])


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 512, 4, 6), (2, 6, 258, 510)], ids=lambda s: "x".join(map(str, s)))
def test_equal_operands_give_exact_zeros(dev, shape):
    f0, _, w, grad_out, _, _ = reference(shape, "independent")
    out, grad = kernel(f0, f0.clone(), w, grad_out, dev)
    assert (out == 0).all() and (grad == 0).all()


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 37, 67), (2, 5, 257, 511)], ids=lambda s: "x".join(map(str, s)))
def test_an_all_zero_pixel_gets_an_exact_zero_gradient(dev, shape):
    """A pixel of f0 that is zero on every channel, and another of f1: the value is the chain's; grad_f0 is exactly 0 at
    the f0 pixel (the chain: NaN, the backward of sqrt at 0), finite everywhere and the chain's everywhere else."""
    f0, f1, w, grad_out, _, _ = reference(shape, "independent")
    f0, f1 = f0.clone(), f1.clone()
    h, wd = shape[2:]
    f0[-1, :, h // 2, wd - 1] = 0
    f1[0, :, h - 1, wd // 3] = 0
    ref32 = chain(f0, f1, w, grad_out, "cuda:0", torch.float32)
    ref64 = chain(f0, f1, w, grad_out, "cpu", torch.float64)
    out, grad = kernel(f0, f1, w, grad_out, dev)
    close(out, ref32[0], rel=True, exact=ref64[0], what=f"{shape} zero pixels out")
    grad = grad.cpu()
    assert torch.isfinite(grad).all()
    assert (grad[-1, :, h // 2, wd - 1] == 0).all()
    assert torch.isnan(ref64[1][-1, :, h // 2, wd - 1]).all()           # the deviation this test is about
    keep = torch.ones(shape[0], 1, h, wd, dtype=torch.bool)
    keep[-1, :, h // 2, wd - 1] = False
    keep = keep.expand(shape)
    assert torch.isfinite(ref64[1][keep]).all() and (grad[0, :, h - 1, wd // 3] != 0).any()
    close(grad[keep], ref32[1][keep], rel=True, exact=ref64[1][keep], what=f"{shape} zero pixels grad_f0")


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 37, 67), (2, 5, 257, 511)], ids=lambda s: "x".join(map(str, s)))
def test_eps_zero_is_served_on_ragged_tiles(dev, shape):
    """eps = 0 with no all-zero pixel: the lanes past the end of the last tile (all three shapes have some) must not
    bring their 0 * (1 / 0) into the sums."""
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, _, _ = reference(shape, "independent")

    def chain0(device, dtype):
        x = f0.to(device=device, dtype=dtype).requires_grad_()
        out = R.level(x, f1.to(device=device, dtype=dtype), w.to(device=device, dtype=dtype), eps=0.0)
        grad, = torch.autograd.grad(out, x, grad_out.to(device=device, dtype=dtype))
        return out.detach().cpu(), grad.cpu()

    x = f0.to(dev).requires_grad_()
    out = WF.lpips_level(x, f1.to(dev), w.to(dev), eps=0.0)
    grad, = torch.autograd.grad(out, x, grad_out.to(dev))
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    compare((out.detach(), grad), chain0("cuda:0", torch.float32), chain0("cpu", torch.float64), f"{shape} eps 0")


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 130, 5, 67), (2, 3, 256, 512)], ids=lambda s: "x".join(map(str, s)))
def test_grad_f1_when_asked(dev, shape):
    f0, f1, w, grad_out, _, _ = reference(shape, "near")
    ref32 = chain(f0, f1, w, grad_out, "cuda:0", torch.float32, both=True)
    ref64 = chain(f0, f1, w, grad_out, "cpu", torch.float64, both=True)
    got = kernel(f0, f1, w, grad_out, dev, both=True)
    compare(got, ref32, ref64, f"{shape} both")
    only = kernel(f0, f1, w, grad_out, dev)
    assert torch.equal(only[0], got[0]) and torch.equal(only[1], got[1])


@pytest.mark.parametrize("shape", [(2, 64, 37, 67), (2, 6, 258, 510)], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(dev, shape):
    f0, f1, w, grad_out, _, _ = reference(shape, "independent")
    first, again = kernel(f0, f1, w, grad_out, dev), kernel(f0, f1, w, grad_out, dev)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_no_host_synchronisation(dev):
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, ref32, ref64 = reference((2, 64, 37, 67), "independent")
    x0, x1, wd, g = f0.to(dev).requires_grad_(), f1.to(dev), w.to(dev), grad_out.to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = WF.lpips_level(x0, x1, wd)
        grad, = torch.autograd.grad(out, x0, g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    compare((out.detach(), grad), ref32, ref64, "under sync debug")


def test_the_framework_routes(dev):
    """fp64 on the device and a trainable ``w`` run the chain in framework ops: no kernel call."""
    from waldo_amd import _lib
    from waldo_amd import functional as WF
    f0, f1, w, _, _, ref64 = reference((3, 5, 7, 9), "independent")
    with _lib.KernelTimer() as timer:
        out64 = WF.lpips_level(f0.to(dev).double(), f1.to(dev).double(), w.to(dev).double())
        out_w = WF.lpips_level(f0.to(dev), f1.to(dev), w.to(dev).requires_grad_())
        assert timer.pairs == {}
        out = WF.lpips_level(f0.to(dev), f1.to(dev), w.to(dev))
    torch.cuda.synchronize()
    assert set(timer.pairs) == {"waldo_lpips_level_fwd"}
    close(out64, ref64[0], rel=True, what="fp64 route")
    assert out_w.requires_grad and out64.dtype == torch.float64 and out.dtype == torch.float32
