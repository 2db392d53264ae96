"""GPU: the 16-bit form of ``WF.plane_norm_gelu`` (waldo_plane_norm_gelu_fwd_dt / _bwd_dt), ``modules.UNet.act_dtype``
and ``WIF.with_unet(opt, act_dtype=...)``, for bf16 and fp16.

The op stores x, skip, the result and grad_x in the 16-bit type T and computes in fp32.  It is compared with its
restatement in framework ops (``WF.plane_norm_gelu_framework``) on the WIDENED operands as leaves, in fp32 (``r32``) and
in fp64 (``exact``).  The bound is derived, not measured: a result stored in T is an fp32 result rounded once to
nearest-even, so per element

    |got - exact| <= B32 + u_T |exact| + tiny_T

with B32 what tests/parity.py::close allows the fp32 op for that tensor (out: TOL + 2 |r32 - exact|; gradients:
TOL scale + 4 |r32 - exact|, the tensor's maximum noise for planes of one or two values, as tests/test_gpu_unet.py
argues), u_T the largest relative error of a rounding to nearest in T (2^-8 for bf16's 8 significant bits, 2^-11 for
fp16's 11) and tiny_T half of fp16's smallest subnormal (2^-25; bf16 has fp32's exponent range: 0).  fp32 results
(grad_weight, grad_bias) take ``close`` as it is.  A store that truncates instead of rounding misses this bound on
several per cent of the elements at every plane from 1 x 2 up; the framework's fp32 result rounded to T stays inside.
The skip slice, grad_skip and the run-to-run comparisons are bit comparisons.

The module and the chain are compared with the framework's own autocast route (``fused = False`` under the same
autocast region), both against the fp64 module: the fused route's rms distance from fp64 may be at most twice the
framework route's own -- both round at the same points, so the two distances are draws of the same rounding noise."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ref as U  # noqa: E402
from parity import TOL, close  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
U_T = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY_T = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}


@pytest.fixture(scope="module")
def WF():
    from waldo_amd import functional
    return functional


@pytest.fixture(autouse=True)
def kernel_at_every_shape(monkeypatch):
    """The launcher's gate sends small planes to the framework ops when a gradient is required: open here, so that every
    test runs the KERNEL."""
    from waldo_amd import functional
    monkeypatch.setattr(functional, "PLANE_NORM_GRAD_FRAMEWORK_HW", ())
    monkeypatch.setattr(functional, "PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP", ())


def close16(got, r32, exact, T, rel=False, what="", noise_of="element"):
    """|got - exact| <= B32 + u_T |exact| + tiny_T per element (the module's docstring); a NaN fails."""
    a, b, e = (t.detach().cpu().double() for t in (got, r32, exact))
    assert a.shape == b.shape == e.shape, (what, a.shape, b.shape, e.shape)
    if a.numel() == 0:
        return
    noise = (b - e).abs()
    if noise_of == "tensor":
        noise = torch.full_like(noise, noise.max().item())
    scale = max(b.abs().max().item(), 1e-30) if rel else 1.0
    bound = TOL * scale + (4.0 if rel else 2.0) * noise + U_T[T] * e.abs() + TINY_T[T]
    err = (a - e).abs()
    ratio = err / bound
    worst = int(ratio.argmax())
    print(f"[parity16] {what}: |hip-ref64| {err.max().item():.3e}  |ref32-ref64| {noise.max().item():.3e}  "
          f"worst {ratio.reshape(-1)[worst].item():.3g} x its bound")
    over = ~(err <= bound)
    if over.any():
        i = int(torch.where(over.reshape(-1), ratio.reshape(-1).nan_to_num(float("inf")), -1.0).argmax())
        raise AssertionError(f"{what}: {int(over.sum())} of {a.numel()} elements beyond their bound; the worst: hip "
                             f"{a.reshape(-1)[i].item():.6e}  ref32 {b.reshape(-1)[i].item():.6e}  ref64 "
                             f"{e.reshape(-1)[i].item():.6e}  bound {bound.reshape(-1)[i].item():.3e}")


def make(dev, T, n, c, cs, h, w, seed, x_pad=0, x_off=0, go_pad=0, mean=0.0):
    """Seeded operands, x / skip / grad_out in T.  ``x_pad``, ``x_off``: x is channels x_off .. x_off + C of a tensor
    with C + x_pad (a batch stride above C H W; x_off: a base that is a channel slice's); ``go_pad``: grad_out is a
    channel slice out of the middle of a larger tensor (not contiguous)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c + x_pad, h, w, generator=g) * 1.5 + mean + 0.3).to(dev, T)[:, x_off:x_off + c]
    weight = (1 + 0.3 * torch.randn(c, generator=g)).to(dev)
    bias = (0.4 * torch.randn(c, generator=g)).to(dev)
    skip = torch.randn(n, cs, h, w, generator=g).to(dev, T) if cs else None
    go = torch.randn(n, c + cs + 2 * go_pad, h, w, generator=g).to(dev, T)[:, go_pad:go_pad + c + cs]
    return x, weight, bias, skip, go


def run_ref(WF, x, weight, bias, skip, go, dtype):
    """(out, grad_x, grad_weight, grad_bias, grad_skip) of the framework ops on the operands widened to ``dtype``."""
    leaves = [None if t is None else t.detach().to(dtype).requires_grad_() for t in (x, weight, bias, skip)]
    out = WF.plane_norm_gelu_framework(*leaves)
    out.backward(go.to(dtype))
    return (out.detach(),) + tuple(None if t is None else t.grad for t in leaves)


def run_op(WF, T, x, weight, bias, skip, go):
    """The same of the op on leaves that keep the operands' types and strides."""
    leaves = [None if t is None else t.detach().requires_grad_() for t in (x, weight, bias, skip)]
    out = WF.plane_norm_gelu(*leaves, out_dtype=T)
    out.backward(go)
    return (out.detach(),) + tuple(None if t is None else t.grad for t in leaves)


def check(WF, T, ops, what):
    x, weight, bias, skip, go = ops
    c = x.shape[1]
    got = run_op(WF, T, *ops)
    r32 = run_ref(WF, *ops, dtype=torch.float32)
    r64 = run_ref(WF, *ops, dtype=torch.float64)
    assert got[0].shape == r32[0].shape
    assert (got[0].dtype, got[1].dtype, got[2].dtype, got[3].dtype) == (T, T, torch.float32, torch.float32), what
    close16(got[0][:, :c], r32[0][:, :c], r64[0][:, :c], T, what=f"{what} out")
    noise_of = "tensor" if x.shape[2] * x.shape[3] <= 2 else "element"   # (tests/test_gpu_unet.py: check)
    close16(got[1], r32[1], r64[1], T, rel=True, what=f"{what} grad_x", noise_of=noise_of)
    for i, name in ((2, "grad_weight"), (3, "grad_bias")):
        assert got[i].shape == r32[i].shape, name
        close(got[i], r32[i], rel=True, exact=r64[i], what=f"{what} {name}", noise_of=noise_of)
    if skip is not None:
        assert got[4].dtype == T
        assert torch.equal(got[0][:, c:], skip), f"{what}: the skip slice is not bit-equal"
        assert torch.equal(got[4], go[:, c:]), f"{what}: grad_skip is not grad_out's slice"
    return got, r64


# planes where a kernel can go wrong: one value, two, odd (element form, 2-byte-aligned channel bases), a multiple of 4
# but not of 8 (the fp32 form's vector width, not this one's), a wavefront's, a workgroup's
PLANES = [(1, 1), (1, 2), (7, 9), (4, 3), (8, 16), (64, 128)]
# (N, C, Cs) dealt over the planes so that every C, N and Cs occurs with small and large planes
MIX = [(1, 1, 0), (3, 3, 1), (1, 32, 5), (3, 1, 5), (1, 3, 0), (3, 32, 1)]


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("i,hw", list(enumerate(PLANES)))
def test_op_against_the_framework_ops(WF, dev, T, i, hw):
    for j in (0, 1, 2):
        n, c, cs = MIX[(2 * i + j) % len(MIX)]
        check(WF, T, make(dev, T, n, c, cs, *hw, seed=10 * i + j), f"{T} {hw} N{n} C{c} Cs{cs}")


@pytest.mark.parametrize("T", DTYPES)
def test_op_on_both_sides_of_every_regime_boundary(WF, dev, T):
    limits = WF.plane_norm_limits()
    assert limits == sorted(limits) and len(limits) >= 2
    k = 0
    for lim in limits:
        for hw in (lim - 1, lim, lim + 1):
            n, c, cs = MIX[k % len(MIX)]
            k += 1
            check(WF, T, make(dev, T, n, min(c, 3), cs, 1, hw, seed=100 + k), f"{T} boundary {lim}: H W = {hw}")
    check(WF, T, make(dev, T, 3, 3, 1, 129, 257, seed=120), f"{T} 129 x 257")   # chunked and odd
    # chunked, vector form, with a partial last chunk
    check(WF, T, make(dev, T, 1, 3, 5, 4, 3 * limits[-1] // 4 + 8, seed=121), f"{T} three chunks and a bit, vector form")


@pytest.mark.parametrize("T", DTYPES)
def test_op_with_strided_operands(WF, dev, T):
    """x with a batch stride above C H W, grad_out a non-contiguous channel slice, x from channel 1 of a 7 x 9 tensor (a
    base that is 2- but not 4-byte aligned): read in place, in every regime."""
    limits = WF.plane_norm_limits()
    for k, (h, w) in enumerate([(7, 9), (8, 16), (1, limits[0] + 8), (1, limits[-1] - 8), (130, 128)]):
        ops = make(dev, T, 3, 3, 1 if k % 2 else 5, h, w, seed=200 + k, x_pad=2, go_pad=1)
        assert not ops[0].is_contiguous() and not ops[4].is_contiguous()
        check(WF, T, ops, f"{T} strided {h} x {w}")
    ops = make(dev, T, 3, 3, 1, 7, 9, seed=206, x_pad=2, x_off=1, go_pad=1)
    assert ops[0].data_ptr() % 4 == 2 and ops[4].data_ptr() % 4 == 2
    check(WF, T, ops, f"{T} 7 x 9 from channel 1")
    x, weight, bias, skip, go = make(dev, T, 3, 3, 0, 6, 10, seed=210)
    rows = x[:, :, ::2]          # planes that are NOT dense: the wrapper copies them
    assert not rows[0, 0].is_contiguous()
    check(WF, T, (rows, weight, bias, None, go[:, :, ::2]), f"{T} rows with a stride")


@pytest.mark.parametrize("T", DTYPES)
def test_a_plane_far_from_zero_keeps_the_bound(WF, dev, T):
    """Mean 100, standard deviation 1 (in T: steps of 1/2 for bf16, 1/16 for fp16): E[x^2] - E[x]^2 in fp32 loses the
    variance; the kernel must not.  The same bound."""
    limits = WF.plane_norm_limits()
    for k, (h, w) in enumerate([(8, 16), (1, limits[1]), (1, limits[-1]), (129, 257)]):
        g = torch.Generator().manual_seed(300 + k)
        x = (100.0 + torch.randn(2, 3, h, w, generator=g)).to(dev, T)
        ops = (x,) + make(dev, T, 2, 3, 0, h, w, seed=310 + k)[1:]
        got, _ = check(WF, T, ops, f"{T} mean 100 at {h} x {w}")
        assert all(bool(torch.isfinite(t.float()).all()) for t in got[:4])


@pytest.mark.parametrize("T", DTYPES)
def test_constant_planes_and_single_values(WF, dev, T):
    """out within the bound of gelu(beta) and every result finite.  (The gradients of a constant plane are what is left
    of a cancellation at rstd = eps^-1/2: the fp32 file does not compare them with the framework's either.)"""
    limits = WF.plane_norm_limits()
    for h, w in [(1, 1), (5, 7), (1, limits[0] + 8), (1, limits[-1] + 5)]:
        x = torch.empty(2, 3, h, w, device=dev, dtype=T)
        for c, v in enumerate((3.75, -100.0, 0.0)):
            x[:, c] = v
        weight = torch.tensor([1.3, -0.7, 2.0], device=dev)
        bias = torch.tensor([0.25, -1.5, 0.8], device=dev)
        go = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(5)).to(dev, T)
        out, gx, gw, gb, _ = run_op(WF, T, x, weight, bias, None, go)
        want = torch.nn.functional.gelu(bias.double()).view(1, 3, 1, 1).expand_as(out)
        close16(out, want, want, T, what=f"{T} constant {h} x {w}")
        assert out.dtype == T and gx.dtype == T
        for t in (out, gx, gw, gb):
            assert bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("T", DTYPES)
def test_results_are_the_same_bits_from_run_to_run_in_both_modes(WF, dev, T):
    import waldo_amd
    limits = WF.plane_norm_limits()
    for k, (h, w) in enumerate([(7, 9), (1, limits[0] + 8), (1, limits[-1]), (129, 257), (4, 3 * limits[-1] // 4 + 8)]):
        ops = make(dev, T, 3, 3, 1, h, w, seed=400 + k)
        first = None
        for mode in (False, True):
            with waldo_amd.deterministic(mode):
                for _ in range(3):
                    got = run_op(WF, T, *ops)
                    if first is None:
                        first = got
                    for a, b in zip(first, got):
                        assert torch.equal(a, b), (h, w, mode)


@pytest.mark.parametrize("T", DTYPES)
def test_out_dtype_under_autocast(WF, dev, T):
    x, weight, bias, skip, go = make(dev, T, 2, 3, 1, 7, 9, seed=500)
    with torch.no_grad():
        outside = WF.plane_norm_gelu(x, weight, bias, skip, out_dtype=T)
        plain = WF.plane_norm_gelu(x, weight, bias, skip)     # a 16-bit x outside autocast: the 16-bit kernel
        want32 = WF.plane_norm_gelu(x.float(), weight, bias, skip.float())
        with torch.autocast("cuda", dtype=T):
            inside = WF.plane_norm_gelu(x, weight, bias, skip, out_dtype=T)
            from32 = WF.plane_norm_gelu(x.float(), weight, bias, skip.float(), out_dtype=T)   # cast to T first
            none = WF.plane_norm_gelu(x, weight, bias, skip)
    assert outside.dtype == T and inside.dtype == T and torch.equal(inside, outside)
    assert plain.dtype == T and torch.equal(plain, outside)
    assert from32.dtype == T and torch.equal(from32, outside)
    assert none.dtype == torch.float32 and torch.equal(none, want32)   # out_dtype=None under autocast: fp32, as ever
    # under autocast with a gradient: the same bits, the gradients in their leaves' types
    leaves = [t.detach().requires_grad_() for t in (x, weight, bias, skip)]
    with torch.autocast("cuda", dtype=T):
        out = WF.plane_norm_gelu(*leaves, out_dtype=T)
    out.backward(go)
    ref = run_op(WF, T, x, weight, bias, skip, go)
    assert torch.equal(out, ref[0])
    for leaf, r in zip(leaves, ref[1:]):
        assert leaf.grad.dtype == r.dtype and torch.equal(leaf.grad, r)


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------
def rms(a, e):
    return (a.detach().double() - e.detach().double()).pow(2).mean().sqrt().item()


def two_x_rule(fused, plain, exact, what):
    """{name: tensor} of the fused route, of the framework's autocast route and of the fp64 module: every tensor of the
    fused route finite and at most twice as far (rms) from fp64 as the framework route's own.  Returns the ratios."""
    ratios = {}
    for k in exact:
        assert bool(torch.isfinite(fused[k].float()).all()), f"{what} {k}"
        d_f, d_p = rms(fused[k], exact[k]), rms(plain[k], exact[k])
        ratios[k] = d_f / d_p if d_p > 0 else (0.0 if d_f == 0 else float("inf"))
        print(f"[2x] {what} {k}: fused {d_f:.3e}  framework {d_p:.3e}  ratio {ratios[k]:.3f}")
    worst = max(ratios, key=ratios.get)
    print(f"[2x] {what}: the largest ratio {ratios[worst]:.3f} ({worst})")
    bad = {k: r for k, r in ratios.items() if not r <= 2.0}
    assert not bad, (what, bad)
    return ratios


def run_net(net, x, go):
    net.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    out = net(x)
    out.backward(go.to(out.dtype))
    res = {"out": out.detach(), "grad_x": x.grad}
    res.update({k: p.grad for k, p in net.named_parameters()})
    return res


@pytest.mark.parametrize("T", DTYPES)
def test_fused_against_the_framework_autocast_route(dev, T):
    from waldo_amd.modules import UNet
    torch.manual_seed(7)
    net = UNet(8, 5, 16, "ln2d", 3, 1, False, "bilinear")
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if ".norm." in k:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    x, go = torch.randn(2, 8, 32, 64, generator=g).to(dev), torch.randn(2, 5, 32, 64, generator=g).to(dev)
    net = net.to(dev)
    net.act_dtype = T
    fused = run_net(net, x, go)
    assert fused["out"].dtype == T and fused["grad_x"].dtype == torch.float32
    assert all(v.dtype == torch.float32 for k, v in fused.items() if k not in ("out", "grad_x"))   # master weights
    net.fused = False
    plain = run_net(net, x, go)
    assert plain["out"].dtype == T
    ref = copy.deepcopy(net).double()
    ref.act_dtype = None
    exact = run_net(ref, x.double(), go.double())
    two_x_rule(fused, plain, exact, f"UNet {T}")


def _fusion(vid, out):
    """The reference's fusion around the network (models/nets/wif.py:49-54, ii_score and ii_ab) in framework ops;
    vid (B, T, Tc, C, H, W) already permuted, out (B, T, Tc, 5, H, W)."""
    score = out[:, :, :, 3:4].softmax(dim=2)
    alpha = (vid[:, :, :, 4:5] + 5).sigmoid()
    return ((alpha * vid[:, :, :, :3] + out[:, :, :, :3]) * score).sum(dim=2)


@pytest.mark.parametrize("T", DTYPES)
def test_wif_with_a_16bit_unet_and_a_16bit_vid(dev, T):
    from waldo_amd.nets import WIF
    from waldo_amd.tools import demo
    opt = demo.demo_opt(dim=16, aspect_ratio=2.0, num_obj=2, num_lyt=5, ii_embed_dim=16, ii_depth=2)
    torch.manual_seed(11)
    wif = WIF.with_unet(opt, act_dtype=T)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        wif.unet.from_emb.weight.normal_(std=0.1, generator=g)   # (zero_init: every output would be the same)
    b, tc, t, c, h, w = 1, 3, 2, 11, 16, 32
    vid = torch.randn(b, tc, t, c, h, w, generator=g).to(dev, T)
    go = torch.randn(b, t, 3, h, w, generator=g).to(dev)
    wif = wif.to(dev)

    def route():
        wif.zero_grad(set_to_none=True)
        out = wif(vid)
        assert out.dtype == torch.float32
        out.backward(go)
        res = {"frames": out.detach()}
        res.update({k: p.grad for k, p in wif.named_parameters()})
        assert all(v.dtype == torch.float32 for v in res.values())
        return res

    fused = route()
    wif.unet.fused = False
    plain = route()
    ref = copy.deepcopy(wif).double()
    ref.unet.act_dtype = None
    v = vid.double().permute(0, 2, 1, 3, 4, 5)
    out = _fusion(v, ref.unet(v.reshape(b * t * tc, c, h, w)).reshape(b, t, tc, -1, h, w))
    out.backward(go.double())
    exact = {"frames": out.detach()}
    exact.update({k: p.grad for k, p in ref.named_parameters()})
    two_x_rule(fused, plain, exact, f"WIF {T}")


@pytest.mark.parametrize("T", DTYPES)
def test_fused_16bit_forward_replays_from_a_graph_with_the_same_bits(dev, T):
    net = U.build("a_", dev)
    net.act_dtype = T
    _, _, d = U.case("a_")
    x = d["x"].to(dev)
    with torch.no_grad():
        eager = net(x).clone()
        assert eager.dtype == T
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
            net(x)
        torch.cuda.current_stream().wait_stream(side)
        static_x = x.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = net(static_x)
        static_x.copy_(torch.zeros_like(x))
        graph.replay()
        zeros = static_out.clone()
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(static_out, eager)
    assert not torch.equal(zeros, eager)   # the replay read its input anew
