"""GPU: the fused warp/composite with a 16-bit (bf16 / fp16) layer stack.  Contract (include/waldo_hip.h): rgb and alpha
have the bits of the fp32 path on ``layers.float()``; grad_layers has the bits of the fp32 gradient ``.to(dtype)``;
the control-point gradient has the fp32 path's bits; grad_occ (float atomics) is held to ``parity.close``.  Unserved
shapes run the fp32 path on the upcast inside the autograd graph.  NaNs are compared by position only."""
import pytest
import torch

from parity import close  # noqa: E402  (tests/parity.py)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
_TPS = {}


def _tps(dev, h, w):
    import waldo_amd
    from waldo_amd.tools.utils import get_grid
    if (h, w) not in _TPS:
        _TPS[(h, w)] = waldo_amd.TPSWarp(h, w, get_grid(4, 4).view(-1, 2)).to(dev)
    return _TPS[(h, w)]


def _rand16(shape, dtype, g):
    """Random finite 16-bit values in [-1, 1] over many binades, with subnormals planted at ~3 % of the elements."""
    x = (torch.rand(shape, generator=g) * 2 - 1) * torch.pow(2.0, -torch.randint(0, 20, shape, generator=g).float())
    x = x.to(dtype)
    mant = 0x7F if dtype == torch.bfloat16 else 0x3FF
    sub = torch.randint(1, mant + 1, shape, generator=g) | (torch.randint(0, 2, shape, generator=g) << 15)
    sub = sub.to(torch.int32).to(torch.int16).view(dtype)
    return torch.where(torch.rand(shape, generator=g) < 0.03, sub, x)


def _inputs(dev, f, nl, h, w, dtype, seed, sigma=0.05):
    from waldo_amd.tools.utils import get_grid
    g = torch.Generator().manual_seed(seed)
    layers = _rand16((f, nl, 4, h, w), dtype, g)
    pts = get_grid(4, 4).view(1, 16, 2) + sigma * torch.randn(f * nl, 16, 2, generator=g)
    s = torch.exp(-torch.randn(f, nl - 1, generator=g) ** 2) + 1e-6
    occ = torch.zeros(f, nl, nl)
    occ[:, 1:, 1:] = s[:, :, None] / (s[:, :, None] + s[:, None, :]) - 0.5 * torch.eye(nl - 1)
    occ[:, 1:, 0] = 1.0
    return layers.to(dev), pts.to(dev), occ.to(dev)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN positions differ ({int((na != nb).sum())})"
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    diff = (a.view(iv) != b.view(iv)) & ~na
    assert not diff.any(), f"{what}: {int(diff.sum())} of {a.numel()} elements differ"


def _call(layers, pts, occ, tps, alpha=True, delta=0.0):
    from waldo_amd import functional as WF
    out = WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t, return_alpha=alpha, delta=delta)
    return out if alpha else (out, None)


def _fwd_bwd(layers, pts, occ, tps, grad_occ, delta, seed=5):
    """Outputs and gradients of the loss (rgb * w).sum() + (alpha * v).sum() with fixed w, v."""
    l2 = layers.detach().clone().requires_grad_()
    p2 = pts.detach().clone().requires_grad_()
    o2 = occ.detach().clone().requires_grad_(grad_occ)
    rgb, alpha = _call(l2, p2, o2, tps, True, delta)
    g = torch.Generator(device=rgb.device).manual_seed(seed)
    w1 = torch.randn(rgb.shape, generator=g, device=rgb.device)
    w2 = torch.randn(alpha.shape, generator=g, device=rgb.device)
    ((rgb * w1).sum() + (alpha * w2).sum()).backward()
    torch.cuda.synchronize()
    return rgb.detach(), alpha.detach(), l2.grad, p2.grad, o2.grad


# ---------------------------------------------------------------------------- 1. forward bits
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("nl", [1, 5, 8, 12, 17, 24, 32])
def test_forward_bits(dev, dtype, nl):
    f, h, w = 2, 32, 64
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, dtype, seed=nl)
    up = layers.float()
    for delta in (0.0, 1.0, 0.5):
        for want_alpha in (True, False):
            # one launch from the control points (no grad, small F) ...
            a = _call(layers, pts, occ, tps, want_alpha, delta)
            b = _call(up, pts, occ, tps, want_alpha, delta)
            # ... and the two-step path (mapping + forward) that a gradient selects
            p2 = pts.clone().requires_grad_()
            c = _call(layers, p2, occ, tps, want_alpha, delta)
            d = _call(up, p2, occ, tps, want_alpha, delta)
            for x, y, what in ((a, b, "pts"), (c, d, "two-step")):
                assert x[0].dtype == torch.float32
                _same_bits(x[0], y[0], f"rgb {what} delta={delta}")
                if want_alpha:
                    _same_bits(x[1], y[1], f"alpha {what} delta={delta}")
            _same_bits(a[0], c[0].detach(), "pts vs two-step")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_forward_bits_violent_warp(dev, dtype):
    """Boxes larger than the LDS image: those layers are gathered straight from the 16-bit planes."""
    f, nl, h, w = 2, 8, 64, 128
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, dtype, seed=3, sigma=0.6)
    for delta in (0.0, 1.0):
        a, b = _call(layers, pts, occ, tps, True, delta), _call(layers.float(), pts, occ, tps, True, delta)
        _same_bits(a[0], b[0], "rgb")
        _same_bits(a[1], b[1], "alpha")
        x, y = _fwd_bwd(layers, pts, occ, tps, True, delta), _fwd_bwd(layers.float(), pts, occ, tps, True, delta)
        _same_bits(x[2], y[2].to(dtype), "grad_layers")
        _same_bits(x[3], y[3], "grad_pts")


# ---------------------------------------------------------------------------- 2. backward bits
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("nl", [1, 5, 8, 12, 17])
def test_backward_bits(dev, dtype, nl):
    f, h, w = 2, 48, 96  # W % 8 == 0: 16-byte gradient stores
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, dtype, seed=100 + nl)
    for grad_occ in (False, True):
        for delta in (0.0, 1.0):
            x = _fwd_bwd(layers, pts, occ, tps, grad_occ, delta)
            y = _fwd_bwd(layers.float(), pts, occ, tps, grad_occ, delta)
            _same_bits(x[0], y[0], "rgb")
            _same_bits(x[1], y[1], "alpha")
            assert x[2].dtype == dtype
            _same_bits(x[2], y[2].to(dtype), f"grad_layers occ={grad_occ} delta={delta}")
            _same_bits(x[3], y[3], "grad_pts")
            if grad_occ:
                close(x[4], y[4], rel=True, what="grad_occ")
            else:
                assert x[4] is None and y[4] is None


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_backward_bits_w_not_multiple_of_8(dev, dtype):
    """W % 8 == 4: the gradient planes go out as 8-byte stores of four texels."""
    f, nl, h, w = 2, 8, 32, 36
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, dtype, seed=77)
    x = _fwd_bwd(layers, pts, occ, tps, False, 0.0)
    y = _fwd_bwd(layers.float(), pts, occ, tps, False, 0.0)
    _same_bits(x[2], y[2].to(dtype), "grad_layers")
    _same_bits(x[3], y[3], "grad_pts")


# ---------------------------------------------------------------------------- 3. fallbacks
def _close16(a16, ref32, dtype, what):
    """A 16-bit gradient from an atomics path: within the 16-bit rounding of the fp32 one (summation order)."""
    assert a16.dtype == dtype
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    close(a16.float(), ref32, tol=eps, rel=True, what=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", ["w70", "l24", "fwd_plain", "bwd_generic"])
def test_fallbacks_keep_the_contract(dev, dtype, case):
    from waldo_amd import _lib
    lib = _lib.load()
    f, nl, h, w = 2, 8, 40, 64
    if case == "w70":
        h, w = 40, 70
    if case == "l24":
        nl = 24
    opt = {"fwd_plain": _lib.DEBUG_FWD_PLAIN, "bwd_generic": _lib.DEBUG_BWD_GENERIC}.get(case)
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, dtype, seed=9)
    try:
        if opt is not None:
            assert lib.waldo_set_debug_option(opt, 1) == 0
        a = _call(layers, pts, occ, tps, True, 0.0)
        b = _call(layers.float(), pts, occ, tps, True, 0.0)
        _same_bits(a[0], b[0], "rgb")
        _same_bits(a[1], b[1], "alpha")
        x = _fwd_bwd(layers, pts, occ, tps, True, 0.0)
        y = _fwd_bwd(layers.float(), pts, occ, tps, True, 0.0)
    finally:
        if opt is not None:
            lib.waldo_set_debug_option(opt, 0)
    _same_bits(x[0], y[0], "rgb (grad)")
    _close16(x[2], y[2], dtype, "grad_layers")
    close(x[3], y[3], rel=True, what="grad_pts")
    close(x[4], y[4], rel=True, what="grad_occ")


# ---------------------------------------------------------------------------- 4. no hidden upcast
def test_no_fp32_copy_of_a_served_stack(dev):
    from torch.utils._python_dispatch import TorchDispatchMode
    f, nl, h, w = 8, 8, 256, 512
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, torch.bfloat16, seed=1)
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            kwargs = kwargs or {}
            if func in (torch.ops.aten._to_copy.default, torch.ops.aten.to.dtype, torch.ops.aten.copy_.default):
                src = args[1] if func is torch.ops.aten.copy_.default else args[0]
                out_dt = args[0].dtype if func is torch.ops.aten.copy_.default else \
                    kwargs.get("dtype", args[1] if len(args) > 1 else None)
                if torch.is_tensor(src) and src.shape == layers.shape and out_dt == torch.float32:
                    seen.append(str(func))
            return func(*args, **(kwargs or {}))

    l2 = layers.clone().requires_grad_()
    p2 = pts.clone().requires_grad_()
    with Watch():
        rgb = _call(l2, p2, occ, tps, False)[0]
        rgb.square().mean().backward()
    torch.cuda.synchronize()
    assert not seen, seen
    assert l2.grad.dtype == torch.bfloat16 and rgb.dtype == torch.float32


# ---------------------------------------------------------------------------- 5. non-finite values
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_nan_and_inf_positions(dev, dtype):
    f, nl, h, w = 2, 8, 64, 64
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, dtype, seed=11)
    layers[0, 3, 1, 20, 30] = float("nan")
    layers[1, 5, 3, 40, 10] = float("inf")
    x = _fwd_bwd(layers, pts, occ, tps, False, 0.0)
    y = _fwd_bwd(layers.float(), pts, occ, tps, False, 0.0)
    assert torch.isnan(x[0]).any() and torch.isnan(x[2]).any()
    _same_bits(x[0], y[0], "rgb")
    _same_bits(x[1], y[1], "alpha")
    _same_bits(x[2], y[2].to(dtype), "grad_layers")


# ---------------------------------------------------------------------------- 6. odd cases
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_zero_frames(dev, dtype):
    tps = _tps(dev, 32, 64)
    layers, pts, occ = _inputs(dev, 1, 8, 32, 64, dtype, seed=2)
    l0 = layers[:0].clone().requires_grad_()
    p0 = pts[:0].clone()
    rgb, alpha = _call(l0, p0, occ[:0], tps, True)
    assert rgb.shape == (0, 3, 32, 64) and alpha.shape == (0, 8, 32, 64) and rgb.dtype == torch.float32
    (rgb.sum() + alpha.sum()).backward()
    assert l0.grad.shape == l0.shape and l0.grad.dtype == dtype


def test_against_the_oracle(dev):
    """One small config against the fp64 / fp32 oracle on the upcast layers (tests/parity.py)."""
    from oracle import wif_oracle as O
    from waldo_amd.tools.utils import get_grid
    f, nl, h, w = 2, 5, 32, 64
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, torch.bfloat16, seed=21)
    rgb, alpha = _call(layers, pts, occ, tps, True)
    inv, rep = O.tps_init(h, w, get_grid(4, 4).view(-1, 2))
    ref = {}
    for dt in (torch.float32, torch.float64):
        ref[dt] = O.warp_composite(layers.cpu().to(dt), pts.cpu().to(dt), occ.cpu().to(dt), inv.to(dt), rep.to(dt))
    close(rgb, ref[torch.float32][0], what="rgb", exact=ref[torch.float64][0], noise_of="tensor")
    close(alpha, ref[torch.float32][1], what="alpha", exact=ref[torch.float64][1], noise_of="tensor")


def test_graph_replay_matches_eager(dev):
    from waldo_amd.graphs import GraphedCall
    f, nl, h, w = 4, 8, 64, 128
    tps = _tps(dev, h, w)
    layers, pts, occ = _inputs(dev, f, nl, h, w, torch.bfloat16, seed=31)
    with torch.no_grad():
        eager = _call(layers, pts, occ, tps, True)
    graphed = GraphedCall(lambda l, p, o: _call(l, p, o, tps, True), layers, pts, occ)
    out = graphed(layers, pts, occ)
    torch.cuda.synchronize()
    _same_bits(out[0], eager[0], "rgb")
    _same_bits(out[1], eager[1], "alpha")
