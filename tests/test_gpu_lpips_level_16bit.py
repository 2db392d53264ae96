"""GPU: ``WF.lpips_level`` on bf16 / fp16 maps with an fp32 ``w`` through its kernels (waldo_lpips_level_fwd_dt /
_bwd_dt, include/waldo_hip.h "LPIPS level distance in 16 bits").

The operands are ``lpips_ref.features(shape, seed, near)`` rounded to the 16-bit type T.  The reference is the chain
(tests/lpips_ref.py) on the WIDENED operands, in fp32 on the device (``r32``) and in fp64 on the CPU (``exact``).  The
bounds are derived, not measured:

  out      an unrounded fp32 result of fp32 arithmetic on exactly widened values: ``parity.close(..., rel=True,
           exact=ref64)`` as it stands for the fp32 kernels.
  grad_f*  the fp32 expression rounded ONCE to nearest-even in T, so tests/test_gpu_unet_16bit.py::close16 with
           rel=True: |got - exact| <= TOL scale + 4 |r32 - exact| + u_T |exact| + tiny_T, u_T = 2^-8 (bf16) / 2^-11
           (fp16), tiny_T = 0 / 2^-25 (half of fp16's smallest subnormal: the gradients of a mean over 10^5 pixels ARE
           fp16 subnormals).  That module's docstring gives the argument; a truncating store misses the bound.

The shapes (N, C, H, W) are the smallest at which each mechanism can fail: one element; P = 63, odd; P = 2479, odd, with
a ragged last tile; channel counts that are no multiple of the four waves or of the backward's 64-channel chunk (65,
130, 512); the five VGG taps of a 32 x 48 frame; P even but no multiple of 4 and P odd with thousands of workgroups;
4200 channels (more than 64 chunks of 64).  Each with independent operands and with f1 = f0 (1 + 1e-2 randn), rounded.

One kernel form ships per dtype (one 2-byte element per lane), chosen from nothing but the dtype: storage that starts
2 bytes past a 4-byte or a 16-byte boundary must therefore give the BITS of aligned storage, which is asserted on top
of the bounds."""
import functools

import pytest
import torch

import lpips_ref as R
from parity import close
from test_gpu_unet_16bit import close16

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
CODE = {torch.float16: 1, torch.bfloat16: 2}   # include/waldo_hip.h: enum waldo_dtype
VGG_TAPS = [(2, 64, 32, 48), (2, 128, 16, 24), (2, 256, 8, 12), (2, 512, 4, 6), (2, 512, 2, 3)]
SHAPES = ([(1, 1, 1, 1), (3, 5, 7, 9), (2, 64, 37, 67), (2, 65, 9, 33), (2, 130, 5, 67), (2, 512, 3, 5)] + VGG_TAPS
          + [(2, 6, 258, 510), (2, 5, 257, 511), (1, 4200, 1, 5)])
KINDS = ("independent", "near")
ODD_START_SHAPES = [(3, 5, 7, 9), (2, 64, 32, 48), (2, 6, 258, 510)]


def ids(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s).replace("torch.", "")


def chain(f0, f1, w, grad_out, device, dtype, both=False, eps=R.EPS):
    """(out, grad_f0[, grad_f1]) of the chain on the operands widened to ``dtype`` on ``device``, back on the CPU."""
    x0 = f0.to(device=device, dtype=dtype).requires_grad_()
    x1 = f1.to(device=device, dtype=dtype).requires_grad_(both)
    out = R.level(x0, x1, w.to(device=device, dtype=dtype), eps=eps)
    grads = torch.autograd.grad(out, (x0, x1) if both else (x0,), grad_out.to(device=device, dtype=dtype))
    return (out.detach().cpu(),) + tuple(g.cpu() for g in grads)


def kernel(f0, f1, w, grad_out, dev, both=False, eps=R.EPS):
    from waldo_amd import functional as WF
    x0 = f0.to(dev).requires_grad_()
    x1 = f1.to(dev).requires_grad_(both)
    out = WF.lpips_level(x0, x1, w.to(dev), eps=eps)
    grads = torch.autograd.grad(out, (x0, x1) if both else (x0,), grad_out.to(dev))
    return (out.detach(),) + grads


@functools.lru_cache(maxsize=None)
def reference(shape, kind, T):
    """The operands rounded to T, a random grad_out per image, and the chain on the widened operands in fp32 on the
    device and fp64 on the CPU: once."""
    f0, f1, w = R.features(shape, seed=sum(shape), near=1e-2 if kind == "near" else None)
    f0, f1 = f0.to(T), f1.to(T)
    grad_out = torch.randn(shape[0], generator=torch.Generator().manual_seed(7)) + 2.0
    ref32 = chain(f0, f1, w, grad_out, "cuda:0", torch.float32)
    ref64 = chain(f0, f1, w, grad_out, "cpu", torch.float64)
    return f0, f1, w, grad_out, ref32, ref64


def compare(got, ref32, ref64, T, what):
    assert got[0].dtype == torch.float32
    close(got[0], ref32[0], rel=True, exact=ref64[0], what=f"{what} out")
    for i, name in enumerate(("grad_f0", "grad_f1")[:len(got) - 1], start=1):
        assert got[i].dtype == T, (what, name, got[i].dtype)
        close16(got[i], ref32[i], ref64[i], T, rel=True, what=f"{what} {name}")


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernel_equals_the_chain_on_the_widened_operands(dev, shape, kind, T):
    f0, f1, w, grad_out, ref32, ref64 = reference(shape, kind, T)
    got = kernel(f0, f1, w, grad_out, dev)
    assert got[0].shape == (shape[0],) and got[1].shape == shape
    compare(got, ref32, ref64, T, f"{shape} {kind} {T}")


def odd_view(t, dev, boundary):
    """``t`` on the device in storage whose first element sits 2 bytes past a 16-byte boundary (``boundary=16``), or 2
    bytes past a 4-byte boundary that is no 16-byte one (``boundary=4``: address 16 k + 6)."""
    n = t.numel()
    buf = torch.empty(n + 16, dtype=t.dtype, device=dev)
    want = 2 if boundary == 16 else 6
    start = ((want - buf.data_ptr() % 16) % 16) // 2
    view = buf[start:start + n].view(t.shape)
    assert view.data_ptr() % 16 == want and view.data_ptr() % 4 == 2 and view.is_contiguous()
    return view.copy_(t)


def direct(x0, x1, w, grad_out, grad):
    """The two entry points on the tensors as they are (dense views): out (N,), and ``grad`` filled."""
    from waldo_amd import _lib
    n, c, h, wd = x0.shape
    p, dev = h * wd, x0.device
    nbytes = _lib.query("waldo_lpips_level_workspace_bytes", n, c, p)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    saved = torch.empty(_lib.query("waldo_lpips_level_saved_bytes", n, c, p) // 4, dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    code = CODE[x0.dtype]
    _lib.launch("waldo_lpips_level_fwd_dt", dev, x0, x1, w, out, saved, ws, nbytes, n, c, p, R.EPS, code)
    _lib.launch("waldo_lpips_level_bwd_dt", dev, x0, x1, w, saved, grad_out, grad, n, c, p, code)
    return out


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("boundary", [4, 16])
@pytest.mark.parametrize("shape", ODD_START_SHAPES, ids=ids)
def test_storage_that_starts_on_an_odd_element(dev, shape, boundary, T):
    """f0, f1 and the gradient buffer each start 2 bytes past a 4-byte (16-byte) boundary: nothing may assume more than
    2-byte alignment, whatever P is.  Through ``WF.lpips_level`` (f0, f1; the gradient is the framework's allocation)
    and through the entry points themselves (the gradient buffer too): the bounds, and the bits of aligned storage.
    The canaries on both sides of the gradient stay untouched."""
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, ref32, ref64 = reference(shape, "independent", T)
    aligned = kernel(f0, f1, w, grad_out, dev)
    x0, x1 = odd_view(f0, dev, boundary).requires_grad_(), odd_view(f1, dev, boundary)
    out = WF.lpips_level(x0, x1, w.to(dev))
    grad, = torch.autograd.grad(out, x0, grad_out.to(dev))
    compare((out.detach(), grad), ref32, ref64, T, f"{shape} odd start {boundary} {T}")
    assert torch.equal(out, aligned[0]) and torch.equal(grad, aligned[1])
    n = f0.numel()
    gbuf = torch.full((n + 32,), 7.0, dtype=T, device=dev)
    want = 2 if boundary == 16 else 6
    start = 8 + ((want - (gbuf.data_ptr() + 16) % 16) % 16) // 2
    gview = gbuf[start:start + n].view(shape)
    assert gview.data_ptr() % 16 == want
    out2 = direct(x0.detach(), x1, w.to(dev), grad_out.to(dev), gview)
    compare((out2, gview), ref32, ref64, T, f"{shape} odd start {boundary} {T}: entry points")
    assert torch.equal(out2, aligned[0]) and torch.equal(gview, aligned[1])
    assert (gbuf[:start] == 7).all() and (gbuf[start + n:] == 7).all()


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 32, 48)], ids=ids)
def test_non_contiguous_operands_are_their_contiguous_copies(dev, shape, T):
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, _, _ = reference(shape, "independent", T)
    want = kernel(f0, f1, w, grad_out, dev)
    x0 = f0.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_()   # channels last
    x1 = torch.stack([f1, f1 + 1], dim=-1).to(dev)[..., 0]                                   # every second element
    assert not x0.is_contiguous() and not x1.is_contiguous()
    out = WF.lpips_level(x0, x1, w.to(dev).view(1, -1, 1, 1))
    grad, = torch.autograd.grad(out, x0, grad_out.to(dev))
    assert torch.equal(out, want[0]) and torch.equal(grad, want[1])


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 512, 4, 6), (2, 6, 258, 510)], ids=ids)
def test_equal_operands_give_exact_zeros(dev, shape, T):
    f0, _, w, grad_out, _, _ = reference(shape, "independent", T)
    out, grad = kernel(f0, f0.clone(), w, grad_out, dev)
    assert (out == 0).all() and (grad == 0).all() and grad.dtype == T


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 37, 67), (2, 5, 257, 511)], ids=ids)
def test_an_all_zero_pixel_gets_an_exact_zero_gradient(dev, shape, T):
    """A pixel of f0 that is zero on every channel, and another of f1: the value is the chain's; grad_f0 is exactly 0 at
    the f0 pixel (the chain: NaN, the backward of sqrt at 0), finite everywhere and the chain's everywhere else."""
    f0, f1, w, grad_out, _, _ = reference(shape, "independent", T)
    f0, f1 = f0.clone(), f1.clone()
    h, wd = shape[2:]
    f0[-1, :, h // 2, wd - 1] = 0
    f1[0, :, h - 1, wd // 3] = 0
    ref32 = chain(f0, f1, w, grad_out, "cuda:0", torch.float32)
    ref64 = chain(f0, f1, w, grad_out, "cpu", torch.float64)
    out, grad = kernel(f0, f1, w, grad_out, dev)
    close(out, ref32[0], rel=True, exact=ref64[0], what=f"{shape} {T} zero pixels out")
    grad = grad.cpu()
    assert torch.isfinite(grad).all()
    assert (grad[-1, :, h // 2, wd - 1] == 0).all()
    assert torch.isnan(ref64[1][-1, :, h // 2, wd - 1]).all()           # the deviation this test is about
    keep = torch.ones(shape[0], 1, h, wd, dtype=torch.bool)
    keep[-1, :, h // 2, wd - 1] = False
    keep = keep.expand(shape)
    assert torch.isfinite(ref64[1][keep]).all() and (grad[0, :, h - 1, wd // 3] != 0).any()
    close16(grad[keep], ref32[1][keep], ref64[1][keep], T, rel=True, what=f"{shape} {T} zero pixels grad_f0")


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 37, 67), (2, 5, 257, 511)], ids=ids)
def test_eps_zero_is_served_on_ragged_tiles(dev, shape, T):
    """eps = 0 with no all-zero pixel: the lanes past the end of the last tile (all three shapes have some) must not
    bring their 0 * (1 / 0) into the sums."""
    f0, f1, w, grad_out, _, _ = reference(shape, "independent", T)
    assert (f0.float().pow(2).sum(1) > 0).all() and (f1.float().pow(2).sum(1) > 0).all()
    got = kernel(f0, f1, w, grad_out, dev, eps=0.0)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    compare(got, chain(f0, f1, w, grad_out, "cuda:0", torch.float32, eps=0.0),
            chain(f0, f1, w, grad_out, "cpu", torch.float64, eps=0.0), T, f"{shape} {T} eps 0")


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 130, 5, 67)], ids=ids)
def test_grad_f1_when_asked(dev, shape, T):
    f0, f1, w, grad_out, _, _ = reference(shape, "near", T)
    ref32 = chain(f0, f1, w, grad_out, "cuda:0", torch.float32, both=True)
    ref64 = chain(f0, f1, w, grad_out, "cpu", torch.float64, both=True)
    got = kernel(f0, f1, w, grad_out, dev, both=True)
    compare(got, ref32, ref64, T, f"{shape} {T} both")
    only = kernel(f0, f1, w, grad_out, dev)
    assert torch.equal(only[0], got[0]) and torch.equal(only[1], got[1])


@pytest.mark.parametrize("T", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(2, 64, 37, 67), (2, 6, 258, 510)], ids=ids)
def test_two_calls_give_the_same_bits(dev, shape, T):
    f0, f1, w, grad_out, _, _ = reference(shape, "independent", T)
    first, again = kernel(f0, f1, w, grad_out, dev), kernel(f0, f1, w, grad_out, dev)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("T", DTYPES, ids=ids)
def test_no_host_synchronisation(dev, T):
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, ref32, ref64 = reference((2, 64, 37, 67), "independent", T)
    x0, x1, wd, g = f0.to(dev).requires_grad_(), f1.to(dev), w.to(dev), grad_out.to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = WF.lpips_level(x0, x1, wd)
        grad, = torch.autograd.grad(out, x0, g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    compare((out.detach(), grad), ref32, ref64, T, f"{T} under sync debug")


@pytest.mark.parametrize("T", DTYPES, ids=ids)
def test_a_graph_replay_gives_the_eager_bits(dev, T):
    """The forward and the backward launch captured once (the entry points on static buffers) and replayed on new
    operands: the bits of the eager call."""
    shape = (2, 64, 37, 67)
    f0, f1, w, grad_out, _, _ = reference(shape, "independent", T)
    eager = kernel(f0, f1, w, grad_out, dev)
    x0, x1, wd, g = torch.zeros(shape, dtype=T, device=dev), f1.to(dev), w.to(dev), grad_out.to(dev)
    grad = torch.empty(shape, dtype=T, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
        direct(x0, x1, wd, g, grad)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = direct(x0, x1, wd, g, grad)
    x0.copy_(f0)
    graph.replay()
    first = (out.clone(), grad.clone())
    graph.replay()
    torch.cuda.synchronize()
    for got in (first, (out, grad)):
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])


@pytest.mark.parametrize("T", DTYPES, ids=ids)
def test_the_routes(dev, T):
    """16-bit maps with an fp32 ``w`` call exactly the ``_dt`` entry points; the same maps with a 16-bit ``w`` or a
    trainable ``w`` call no kernel; fp32 operands still call the fp32 entry point."""
    from waldo_amd import _lib
    from waldo_amd import functional as WF
    f0, f1, w, grad_out, ref32, ref64 = reference((3, 5, 7, 9), "independent", T)
    x0, x1, wd, g = f0.to(dev), f1.to(dev), w.to(dev), grad_out.to(dev)
    with _lib.KernelTimer() as timer:
        out = WF.lpips_level(x0, x1, wd)
        torch.cuda.synchronize()
        assert set(timer.pairs) == {"waldo_lpips_level_fwd_dt"} and len(timer.pairs["waldo_lpips_level_fwd_dt"]) == 1
        leaf = x0.clone().requires_grad_()
        grad, = torch.autograd.grad(WF.lpips_level(leaf, x1, wd), leaf, g)
        torch.cuda.synchronize()
        assert {k: len(v) for k, v in timer.pairs.items()} == {"waldo_lpips_level_fwd_dt": 2, "waldo_lpips_level_bwd_dt": 1}
    compare((out, grad), ref32, ref64, T, f"{T} routes")
    with _lib.KernelTimer() as timer:
        same = WF.lpips_level(x0, x1, wd.to(T))
        leaf, wt = x0.clone().requires_grad_(), wd.clone().requires_grad_()
        out_w = WF.lpips_level(leaf, x1, wt)
        g_leaf, g_w = torch.autograd.grad(out_w, (leaf, wt), g)
        torch.cuda.synchronize()
        assert timer.pairs == {}
        out32 = WF.lpips_level(x0.float(), x1.float(), wd)
    torch.cuda.synchronize()
    assert set(timer.pairs) == {"waldo_lpips_level_fwd"}
    assert same.dtype == T and torch.equal(same, WF.lpips_level_framework(x0, x1, wd.to(T)))
    assert out_w.dtype == torch.float32 and g_leaf.dtype == T and g_w.dtype == torch.float32
    close(out_w, ref32[0], rel=True, exact=ref64[0], what=f"{T} trainable w out")
    close16(g_leaf, ref32[1], ref64[1], T, rel=True, what=f"{T} trainable w grad_f0")
    close(out32, ref32[0], rel=True, exact=ref64[0], what=f"{T} fp32 route on the widened maps")
    assert torch.equal(out32, out)   # the same arithmetic on the same widened values, whatever the storage
