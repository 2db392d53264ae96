"""GPU: ``WF.plane_norm_gelu`` (waldo_plane_norm_gelu_fwd / _bwd), ``waldo_amd.modules.UNet`` and ``WIF.with_unet``.

The op is compared with its restatement in framework ops (``WF.plane_norm_gelu_framework``: GroupNorm with one group per
channel, the exact GELU, torch.cat) run on the same device in fp32 and, as ``exact``, in fp64; the bounds are the
project's (tests/parity.py::close: TOL plus the measured fp32 noise of the restatement).  The skip slice and the
run-to-run comparisons are bit comparisons.  The module is compared with the fixture recorded from the reference's own
UNet (tests/golden/unet_reference.npz)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ref as U  # noqa: E402
from parity import TOL, close  # noqa: E402

from waldo_amd import functional as _functional  # noqa: E402

pytestmark = pytest.mark.gpu
# (read before any test opens the gate)
SHIPPED_GATE = (_functional.PLANE_NORM_GRAD_FRAMEWORK_HW, _functional.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP)


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


def make(dev, n, c, cs, h, w, seed, x_pad=0, go_pad=0, mean=0.0):
    """Seeded operands.  ``x_pad``: x is the first C channels of a tensor with C + x_pad (a batch stride above C H W);
    ``go_pad``: grad_out is a channel slice out of the middle of a larger tensor (not contiguous)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c + x_pad, h, w, generator=g) * 1.5 + mean + 0.3).to(dev)[:, :c]
    weight = (1 + 0.3 * torch.randn(c, generator=g)).to(dev)
    bias = (0.4 * torch.randn(c, generator=g)).to(dev)
    skip = torch.randn(n, cs, h, w, generator=g).to(dev) if cs else None
    go = torch.randn(n, c + cs + 2 * go_pad, h, w, generator=g).to(dev)[:, go_pad:go_pad + c + cs]
    assert x.is_contiguous() == (x_pad == 0 or n == 1) and go.is_contiguous() == (go_pad == 0 or n == 1)
    return x, weight, bias, skip, go


def run(fn, x, weight, bias, skip, go, dtype=torch.float32):
    """(out, grad_x, grad_weight, grad_bias, grad_skip) of ``fn`` on leaves that keep the operands' strides."""
    leaves = [None if t is None else t.detach().to(dtype).requires_grad_() for t in (x, weight, bias, skip)]
    out = fn(*leaves)
    out.backward(go.to(dtype))
    return (out.detach(),) + tuple(None if t is None else t.grad for t in leaves)


def check(WF, ops, what):
    x, weight, bias, skip, go = ops
    c = x.shape[1]
    got = run(WF.plane_norm_gelu, *ops)
    r32 = run(WF.plane_norm_gelu_framework, *ops)
    r64 = run(WF.plane_norm_gelu_framework, *ops, dtype=torch.float64)
    assert got[0].shape == r32[0].shape and got[0].dtype == torch.float32
    close(got[0][:, :c], r32[0][:, :c], exact=r64[0][:, :c], what=f"{what} out")
    # gradients: per element, as everywhere.  Planes of ONE or TWO values alone take the restatement's noise over the
    # tensor (parity.close: "... moves elements whose own fp32 noise happens to be small"): removing the mean and the
    # projection on xhat takes both degrees of freedom of two values, so grad_x is what is left when terms of the size of
    # rstd gamma dz cancel -- (var + eps) / eps ~ 1e5 times smaller than they are -- and every fp32 evaluation, the
    # framework's too, is a per cent of such an element away from exact; which element the framework happens to get
    # right to 0.1 % says nothing about the kernel.  From three values on a plane keeps a gradient of the terms' size.
    noise_of = "tensor" if x.shape[2] * x.shape[3] <= 2 else "element"
    for i, name in ((1, "grad_x"), (2, "grad_weight"), (3, "grad_bias")):
        assert got[i].shape == r32[i].shape, name
        close(got[i], r32[i], rel=True, exact=r64[i], what=f"{what} {name}", noise_of=noise_of)
    if skip is not None:
        assert torch.equal(got[0][:, c:], skip), f"{what}: the skip slice is not bit-equal"
        assert torch.equal(got[4], go[:, c:]), f"{what}: grad_skip is not grad_out's slice"
    return got


# planes where a kernel can go wrong: one value, two, no vector width (7 x 9), a wavefront's, a workgroup's
PLANES = [(1, 1), (1, 2), (7, 9), (8, 16), (64, 128)]
# (N, C, Cs) dealt over the planes so that every C, N and Cs occurs with small and large planes
MIX = [(1, 1, 0), (3, 3, 1), (1, 32, 5), (3, 1, 5), (1, 3, 0), (3, 32, 1)]


@pytest.mark.parametrize("i,hw", list(enumerate(PLANES)))
def test_op_against_the_framework_ops(WF, dev, i, hw):
    for j in (0, 1, 2):
        n, c, cs = MIX[(2 * i + j) % len(MIX)]
        check(WF, make(dev, n, c, cs, *hw, seed=10 * i + j), f"{hw} N{n} C{c} Cs{cs}")


def test_op_on_both_sides_of_every_regime_boundary(WF, dev):
    limits = WF.plane_norm_limits()
    assert limits == sorted(limits) and len(limits) >= 2
    k = 0
    for lim in limits:
        for hw in (lim - 1, lim, lim + 1):
            n, c, cs = MIX[k % len(MIX)]
            k += 1
            check(WF, make(dev, n, min(c, 3), cs, 1, hw, seed=100 + k), f"boundary {lim}: H W = {hw}")
    # vector and scalar forms of the chunked regime, with a last chunk that is partial
    check(WF, make(dev, 3, 3, 1, 129, 257, seed=120), "129 x 257")
    check(WF, make(dev, 1, 3, 5, 4, 3 * limits[-1] // 4 + 4, seed=121), "three chunks and a bit, vector form")


def test_op_with_strided_operands(WF, dev):
    """x with a batch stride above C H W, grad_out a non-contiguous channel slice: read in place, in every regime."""
    limits = WF.plane_norm_limits()
    for k, (h, w) in enumerate([(7, 9), (8, 16), (1, limits[0] + 4), (1, limits[-1] - 8), (130, 128)]):
        ops = make(dev, 3, 3, 1 if k % 2 else 5, h, w, seed=200 + k, x_pad=2, go_pad=1)
        check(WF, ops, f"strided {h} x {w}")
    x, weight, bias, skip, go = make(dev, 3, 3, 0, 6, 10, seed=210)
    rows = x[:, :, ::2]          # planes that are NOT dense: the wrapper copies them
    assert not rows[0, 0].is_contiguous()
    check(WF, (rows, weight, bias, None, go[:, :, ::2]), "rows with a stride")


def test_a_plane_far_from_zero_keeps_the_bound(WF, dev):
    """Mean 100, standard deviation 1: E[x^2] - E[x]^2 in fp32 loses the variance; the kernel must not."""
    limits = WF.plane_norm_limits()
    for k, (h, w) in enumerate([(8, 16), (1, limits[1]), (1, limits[-1]), (129, 257)]):
        g = torch.Generator().manual_seed(300 + k)
        x = (100.0 + torch.randn(2, 3, h, w, generator=g)).to(dev)
        ops = (x,) + make(dev, 2, 3, 0, h, w, seed=310 + k)[1:]
        got = check(WF, ops, f"mean 100 at {h} x {w}")
        r64 = run(WF.plane_norm_gelu_framework, *ops, dtype=torch.float64)
        err = (got[0].double() - r64[0]).abs().max().item()
        ex2 = (x * x).mean(dim=(2, 3), keepdim=True) - x.mean(dim=(2, 3), keepdim=True) ** 2  # the naive form, fp32
        naive = torch.nn.functional.gelu((x - x.mean(dim=(2, 3), keepdim=True)) * torch.rsqrt(ex2 + 1e-5)
                                         * ops[1].view(1, -1, 1, 1) + ops[2].view(1, -1, 1, 1))
        naive_err = (naive.double() - r64[0]).abs().max().item()
        print(f"[conditioning] {h} x {w}: |kernel - fp64| {err:.2e}; the naive variance in fp32: {naive_err:.2e}")
        assert err <= TOL, (h, w, err)   # against exact arithmetic alone, whatever the fp32 restatement's own noise
        assert naive_err > TOL, (h, w, naive_err)   # the data discriminates: the naive form misses the same bound


def test_constant_planes_and_single_values(WF, dev):
    limits = WF.plane_norm_limits()
    for h, w in [(1, 1), (5, 7), (1, limits[0] + 3), (1, limits[-1] + 5)]:
        x = torch.empty(2, 3, h, w, device=dev)
        for c, v in enumerate((3.7, -100.0, 0.0)):
            x[:, c] = v
        weight = torch.tensor([1.3, -0.7, 2.0], device=dev)
        bias = torch.tensor([0.25, -1.5, 0.8], device=dev)
        go = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(5)).to(dev)
        out, gx, gw, gb, _ = run(WF.plane_norm_gelu, x, weight, bias, None, go)
        want = torch.nn.functional.gelu(bias.double()).view(1, 3, 1, 1).expand_as(out)
        close(out, want, what=f"constant {h} x {w}")
        for t in (gx, gw, gb):
            assert bool(torch.isfinite(t).all())


def test_results_are_the_same_bits_from_run_to_run_in_both_modes(WF, dev):
    import waldo_amd
    limits = WF.plane_norm_limits()
    for k, (h, w) in enumerate([(7, 9), (1, limits[0] + 4), (1, limits[-1]), (129, 257)]):
        ops = make(dev, 3, 3, 1, h, w, seed=400 + k)
        first = None
        for mode in (False, True):
            with waldo_amd.deterministic(mode):
                for _ in range(3):
                    got = run(WF.plane_norm_gelu, *ops)
                    if first is None:
                        first = got
                    for a, b in zip(first, got):
                        assert torch.equal(a, b), (h, w, mode)


def test_autocast_computes_in_fp32(WF, dev):
    x, weight, bias, skip, go = make(dev, 2, 3, 1, 7, 9, seed=500)
    want = WF.plane_norm_gelu(x.bfloat16().float(), weight, bias, skip.bfloat16().float())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = WF.plane_norm_gelu(x.bfloat16(), weight, bias, skip.bfloat16())
    assert got.dtype == torch.float32 and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", U.CASES)
def test_unet_equals_the_reference_fixture_on_the_device(dev, prefix):
    _, keys, d = U.case(prefix)
    net = U.build(prefix, dev)
    got = U.run(net, d["x"].to(dev), d["grad_out"].to(dev))
    U.check(close, got, d, keys, f"gpu {prefix}")


def test_fused_against_unfused_on_the_device(dev):
    from waldo_amd.modules import UNet
    torch.manual_seed(7)
    net = UNet(8, 5, 16, "ln2d", 3, 1, False, "bilinear")
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if ".norm." in k:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    x, go = torch.randn(2, 8, 32, 64, generator=g), torch.randn(2, 5, 32, 64, generator=g)
    net = net.to(dev)
    fused = U.run(net, x.to(dev), go.to(dev))
    net.fused = False
    plain = U.run(net, x.to(dev), go.to(dev))
    exact = U.run(net.double(), x.double().to(dev), go.double().to(dev))
    close(fused[0], plain[0], rel=True, exact=exact[0], what="out")
    close(fused[1], plain[1], rel=True, exact=exact[1], what="grad_x")
    for k in plain[2]:
        close(fused[2][k], plain[2][k], rel=True, exact=exact[2][k], what=k)


def test_the_gate_as_shipped_changes_no_result_beyond_parity(WF, dev, monkeypatch):
    """The same module with the gate open and as it ships (small planes under autograd on the framework ops)."""
    _, keys, d = U.case("a_")
    net = U.build("a_", dev)
    opened = U.run(net, d["x"].to(dev), d["grad_out"].to(dev))
    monkeypatch.setattr(WF, "PLANE_NORM_GRAD_FRAMEWORK_HW", SHIPPED_GATE[0])
    monkeypatch.setattr(WF, "PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP", SHIPPED_GATE[1])
    for lo, hi in SHIPPED_GATE[0] + SHIPPED_GATE[1]:
        assert 1 <= lo <= hi < 256 * 512  # the large levels, where the traffic is, are never gated
    got = U.run(net, d["x"].to(dev), d["grad_out"].to(dev))
    U.check(close, got, d, keys, "gate as shipped")
    close(got[0], opened[0], rel=True, what="shipped against open")


def _fusion(vid, out):
    """The reference's fusion around the network (models/nets/wif.py:49-54, ii_score and ii_ab) in framework ops;
    vid (B, T, Tc, C, H, W) already permuted, out (B, T, Tc, 5, H, W)."""
    score = out[:, :, :, 3:4].softmax(dim=2)
    alpha = (vid[:, :, :, 4:5] + 5).sigmoid()
    return ((alpha * vid[:, :, :, :3] + out[:, :, :, :3]) * score).sum(dim=2)


def test_wif_with_unet_forward_and_backward_against_the_cpu_route(dev):
    from waldo_amd.nets import WIF
    from waldo_amd.tools import demo
    opt = demo.demo_opt(dim=16, aspect_ratio=2.0, num_obj=2, num_lyt=5, ii_embed_dim=16, ii_depth=2)
    torch.manual_seed(11)
    wif = WIF.with_unet(opt)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        wif.unet.from_emb.weight.normal_(std=0.1, generator=g)   # (zero_init: every output would be the same)
    b, tc, t, c, h, w = 1, 3, 2, 11, 16, 32
    vid = torch.randn(b, tc, t, c, h, w, generator=g)
    go = torch.randn(b, t, 3, h, w, generator=g)

    def cpu_route(dtype):
        net = WIF.with_unet(opt).to(dtype)
        net.load_state_dict({k: v.to(dtype) for k, v in wif.state_dict().items()}, strict=True)
        v = vid.to(dtype).permute(0, 2, 1, 3, 4, 5)
        out = _fusion(v, net.unet(v.reshape(b * t * tc, c, h, w)).reshape(b, t, tc, -1, h, w))
        out.backward(go.to(dtype))
        return out.detach(), {k: p.grad for k, p in net.named_parameters()}

    r32, r64 = cpu_route(torch.float32), cpu_route(torch.float64)
    wif = wif.to(dev)
    out = wif(vid.to(dev))
    out.backward(go.to(dev))
    close(out, r32[0], rel=True, exact=r64[0], what="WIF.forward")
    for k, p in wif.named_parameters():
        close(p.grad, r32[1][k], rel=True, exact=r64[1][k], what=k)


def test_fused_unet_forward_replays_from_a_graph_with_the_same_bits(dev):
    net = U.build("a_", dev)
    _, _, d = U.case("a_")
    x = d["x"].to(dev)
    with torch.no_grad():
        eager = net(x).clone()
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
