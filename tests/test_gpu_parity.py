"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the golden vectors.

Tolerance: BASELINE.json north_star -- outputs within 1e-4 fp32 of the reference on identical
inputs.  Gradients are sums of many such terms; they are checked to 1e-4 RELATIVE to the
largest gradient magnitude of the tensor (float atomics reorder the sums).
"""
import pytest
import torch

from oracle import wif_oracle as O

pytestmark = pytest.mark.gpu

from parity import TOL, close, compare_warp_composite  # noqa: E402  (tests/parity.py: 1e-4 + the measured fp32 noise of the reference)


def test_native_library_is_loaded(dev):
    from waldo_amd import _lib
    lib = _lib.load()
    assert lib.waldo_version() >= 1000
    maps = open("/proc/self/maps").read()
    assert "libwaldo_hip.so" in maps


# ----------------------------------------------------------------------------- A2
@pytest.mark.parametrize("tag", ["k16", "k32"])
def test_tps_golden(dev, golden, tag):
    import waldo_amd
    g = golden(f"tps_{tag}")
    h, w = int(g["h"]), int(g["w"])
    mod = waldo_amd.TPSWarp(h, w, g["ctrl"])
    # init-time buffers come from an fp32 torch.inverse on the HOST of an ill-conditioned matrix:
    # they differ between hosts by up to ~1e-4 relative (LAPACK code paths), so they are close,
    # not bit-equal, across machines ...
    close(mod.inverse_kernel, g["inverse_kernel"], 1e-3, rel=True, what="inverse_kernel")
    close(mod.tgt_grid_repr, g["tgt_grid_repr"], 1e-6, what="tgt_grid_repr")
    # ... and parity is checked the way the drop-in is used: with the reference's buffers loaded
    mod.load_state_dict({"inverse_kernel": g["inverse_kernel"], "tgt_grid_repr": g["tgt_grid_repr"]},
                        strict=False)
    mod = mod.to(dev)
    assert torch.equal(mod.basis_t.cpu(), g["tgt_grid_repr"].t())
    pts = g["pts"].to(dev).requires_grad_()
    grid = mod(pts)
    p64 = g["pts"].double().requires_grad_()
    g64 = O.tps_grid(g["inverse_kernel"].double(), g["tgt_grid_repr"].double(), p64, h, w)
    (g64 * g["wgt"].double()).sum().backward()
    close(grid, g["grid"], what="grid", exact=g64)
    (grid * g["wgt"].to(dev)).sum().backward()
    close(pts.grad, g["grad_pts"], rel=True, what="grad_pts", exact=p64.grad)


def test_tps_bg_sized(dev):
    """Background-sized TPS of the real recipe: N = 128 control points (8x16), K3 = 131."""
    import waldo_amd
    ctrl = O.get_grid(8, 16).view(-1, 2)
    h, w = 32, 64
    mod = waldo_amd.TPSWarp(h, w, ctrl).to(dev)
    inv, rep = mod.inverse_kernel.cpu(), mod.tgt_grid_repr.cpu()  # same host, same buffers
    torch.manual_seed(0)
    pts = (ctrl.view(1, -1, 2) + 0.02 * torch.randn(11, 128, 2)).requires_grad_()
    ref = O.tps_grid(inv, rep, pts, h, w)
    wgt = torch.randn(ref.shape)
    (ref * wgt).sum().backward()
    p64 = pts.detach().double().requires_grad_()
    ref64 = O.tps_grid(inv.double(), rep.double(), p64, h, w)
    (ref64 * wgt.double()).sum().backward()
    p2 = pts.detach().to(dev).requires_grad_()
    out = mod(p2)
    close(out, ref, what="grid", exact=ref64)
    (out * wgt.to(dev)).sum().backward()
    close(p2.grad, pts.grad, rel=True, what="grad_pts", exact=p64.grad, noise_of="tensor")


def test_tps_identity(dev):
    import waldo_amd
    ctrl = O.get_grid(4, 4).view(-1, 2)
    mod = waldo_amd.TPSWarp(24, 40, ctrl).to(dev)
    out = mod(ctrl.view(1, 16, 2).to(dev))
    close(out, O.get_grid(24, 40), 1e-5)


# ----------------------------------------------------------------------------- A4/A5
@pytest.mark.parametrize("delta", [0, 1])
def test_grid_sample_golden(dev, golden, delta):
    from waldo_amd import functional as WF
    g = golden(f"grid_sample_d{delta}")
    x = g["x"].to(dev).requires_grad_()
    grid = g["grid"].to(dev).requires_grad_()
    out = WF.grid_sample(x, grid, delta=float(g["delta"]))
    close(out, g["out"], what="out")
    (out * g["wgt"].to(dev)).sum().backward()
    close(x.grad, g["grad_x"], rel=True, what="grad_x")
    close(grid.grad, g["grad_grid"], rel=True, what="grad_grid")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1, 1), (2, 3, 7, 5, 300, 1), (4, 2, 64, 64, 128, 256),
                                   (6, 23, 16, 32, 16, 32),
                                   (2, 2, 128, 256, 40, 32), (1, 40, 64, 128, 8, 8)])
def test_grid_sample_random(dev, shape):
    from waldo_amd import functional as WF
    n, c, hi, wi, ho, wo = shape
    torch.manual_seed(n * 7 + c)
    x = torch.randn(n, c, hi, wi, requires_grad=True)
    grid = (torch.rand(n, ho, wo, 2) * 2.4 - 1.2).requires_grad_()
    ref = O.grid_sample_delta(x, grid, 0.5)
    wgt = torch.randn(ref.shape)
    (ref * wgt).sum().backward()
    x2, g2 = x.detach().to(dev).requires_grad_(), grid.detach().to(dev).requires_grad_()
    out = WF.grid_sample(x2, g2, delta=0.5)
    close(out, ref, what="out")
    (out * wgt.to(dev)).sum().backward()
    close(x2.grad, x.grad, rel=True, what="grad_x")
    close(g2.grad, grid.grad, rel=True, what="grad_grid")


def test_grid_sample_broadcast(dev):
    """Input expanded over time as in Warper.obj_to_output (lvd.py:544): (B,1,No,..) -> (B,T,No,..)"""
    from waldo_amd import functional as WF
    b, t, no, c, ho, wo, h, w = 2, 3, 4, 2, 8, 8, 12, 10
    torch.manual_seed(3)
    obj = torch.randn(b, no, c, ho, wo, requires_grad=True)
    grid = (torch.rand(b * t * no, h, w, 2) * 2.2 - 1.1)
    exp = obj.view(b, 1, no, c, ho, wo).expand(-1, t, -1, -1, -1, -1).reshape(b * t * no, c, ho, wo)
    ref = O.grid_sample_delta(exp, grid, 1.0)
    wgt = torch.randn(ref.shape)
    (ref * wgt).sum().backward()
    o2 = obj.detach().to(dev).requires_grad_()
    out = WF.grid_sample(o2.view(b * no, c, ho, wo), grid.to(dev), delta=1.0, broadcast=(t * no, no))
    close(out, ref, what="out")
    (out * wgt.to(dev)).sum().backward()
    close(o2.grad, obj.grad, rel=True, what="grad_obj")


@pytest.mark.parametrize("hwo", [(12, 10), (16, 32)])   # one pixel per thread / four (Ho * Wo % 4 == 0)
def test_grid_sample_mask_by_product(dev, hwo):
    """waldo_grid_sample2d_ex_fwd: the output is the plain call's, and the mask is grid_sample(ones, grid) -- the
    warped all-ones canvas of Warper.grid_to_flow_ctx's ghost test (lvd.py:785-791) -- bit for bit; with the input
    expanded over time, with the grid repeated over the contexts, and under autograd (the mask carries none).  And
    its output slots: two calls fill the concatenated (frames, L, C, H, W) tensor of Warper.layer_to_output."""
    from waldo_amd import _lib, functional as WF
    b, t, no, c, ho, wo = 2, 3, 4, 2, 8, 8
    h, w = hwo
    torch.manual_seed(4)
    obj = torch.randn(b * t * no, c, ho, wo, device=dev)
    grid = (torch.rand(b * t * no, h, w, 2, device=dev) * 2.6 - 1.3)
    ones = torch.ones(b * t * no, 1, ho, wo, device=dev)
    with torch.no_grad():
        out, mask = WF.grid_sample(obj, grid, delta=0.0, return_mask=True)
        assert torch.equal(out, WF.grid_sample(obj, grid, delta=0.0))
        assert torch.equal(mask, WF.grid_sample(ones, grid, delta=0.0))
        assert 0.05 < (mask > 0.9).float().mean().item() < 0.95   # the grid leaves the canvas in places
        # input shared over time
        out, mask = WF.grid_sample(obj[:b * no], grid, delta=1.0, broadcast=(t * no, no), return_mask=True)
        assert torch.equal(out, WF.grid_sample(obj[:b * no], grid, delta=1.0, broadcast=(t * no, no)))
        assert torch.equal(mask, WF.grid_sample(ones, grid, delta=0.0))
        # grid repeated over two contexts
        rep = 2
        big = torch.randn(b * rep * t * no, c, ho, wo, device=dev)
        gr = (b * rep * t * no, rep * t * no, t * no)
        out, mask = WF.grid_sample(big, grid, grid_repeat=gr, return_mask=True)
        assert torch.equal(out, WF.grid_sample(big, grid, grid_repeat=gr))
        assert torch.equal(mask, WF.grid_sample(torch.ones(b * rep * t * no, 1, ho, wo, device=dev), grid, grid_repeat=gr))
        # output slots: the background (one map per frame) and the objects (No per frame) written straight into the
        # tensor Warper.layer_to_output's torch.cat would build
        frames = b * t
        bgmap = torch.randn(frames, c, ho, wo, device=dev)
        bggrid = (torch.rand(frames, h, w, 2, device=dev) * 2.6 - 1.3)
        want = torch.cat([WF.grid_sample(bgmap, bggrid).view(frames, 1, c, h, w),
                          WF.grid_sample(obj, grid).view(frames, no, c, h, w)], dim=1)
        dst = torch.full((frames, no + 1, c, h, w), float("nan"), device=dev)
        assert WF.grid_sample(bgmap, bggrid, out=(dst, 1, no + 1, 0)) is dst
        _, mask = WF.grid_sample(obj, grid, return_mask=True, out=(dst, no, no + 1, 1))
        assert torch.equal(dst, want) and torch.equal(mask, WF.grid_sample(ones, grid, delta=0.0))
        with pytest.raises(_lib.WaldoHipError):
            WF.grid_sample(obj, grid, out=(dst, no, no, 1))          # offset + group > stride
        with pytest.raises(_lib.WaldoHipError):
            WF.grid_sample(obj, grid, out=(dst[:1], no, no + 1, 1))  # too small
    x, g = obj.clone().requires_grad_(), grid.clone().requires_grad_()
    out, mask = WF.grid_sample(x, g, return_mask=True)
    assert not mask.requires_grad
    (out.square().sum() + mask.sum()).backward()
    x2, g2 = obj.clone().requires_grad_(), grid.clone().requires_grad_()
    WF.grid_sample(x2, g2).square().sum().backward()
    assert torch.equal(g.grad, g2.grad)
    close(x.grad, x2.grad, 1e-5, rel=True, what="grad_input (float atomics: order of additions)")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hwo", [(12, 10), (16, 32)])
def test_layers_to_output_is_the_concatenation(dev, hwo, shared):
    """WF.layers_to_output = Warper.layer_to_output (lvd.py:533-559) as one differentiable op.  With pre = (1, 0)
    its forward has the bits of `cat([grid_sample(bg), grid_sample(obj)])`, its grid gradients too (they are written,
    not accumulated), its image gradients agree up to the order of the float atomics; with pre = (0.5, 0.5) it is
    `cat(...)` of `(x + 1) / 2` (grid_to_flow's rough alphas, lvd.py:602-606) to rounding, values and gradients;
    against the CPU restatement as well.  `shared`: the images shared over time (lvd.py:544,555)."""
    from waldo_amd import _lib, functional as WF
    b, t, no, c, ho, wo = 2, 3, 4, 2, 8, 8
    h, w = hwo
    frames = b * t
    torch.manual_seed(5)
    obj = torch.randn(b * no if shared else frames * no, c, ho, wo, device=dev)
    bg = torch.randn(b if shared else frames, c, h, w, device=dev)
    gobj = torch.rand(frames * no, h, w, 2, device=dev) * 2.6 - 1.3
    gbg = torch.rand(frames, h, w, 2, device=dev) * 2.6 - 1.3
    obc, bbc = ((t * no, no), (t, 1)) if shared else (None, None)
    wgt = torch.randn(frames, no + 1, c, h, w, device=dev)

    def spelled(pre, delta):
        leaves = [x.clone().requires_grad_() for x in (obj, bg, gobj, gbg)]
        o, g, go, gb = leaves
        oo, gg = (o, g) if pre is None else ((o + 1) / 2, (g + 1) / 2)
        out = torch.cat([WF.grid_sample(gg, gb, delta=delta, broadcast=bbc).view(frames, 1, c, h, w),
                         WF.grid_sample(oo, go, delta=delta, broadcast=obc).view(frames, no, c, h, w)], dim=1)
        (out * wgt).sum().backward()
        return out.detach(), [x.grad for x in leaves]

    def fused(pre, delta, mask=False):
        leaves = [x.clone().requires_grad_() for x in (obj, bg, gobj, gbg)]
        o, g, go, gb = leaves
        out = WF.layers_to_output(o, g, go, gb, delta, delta, obc, bbc, pre if pre is not None else (1.0, 0.0), mask)
        out, m = out if mask else (out, None)
        (out * wgt).sum().backward()
        return out.detach(), [x.grad for x in leaves], m

    for delta in (0.0, 1.0):
        want, wg = spelled(None, delta)
        got, gg, mask = fused(None, delta, mask=True)
        assert torch.equal(got, want)
        assert torch.equal(gg[2], wg[2]) and torch.equal(gg[3], wg[3])
        close(gg[0], wg[0], 1e-5, rel=True, what="grad_obj (float atomics: order of additions)")
        close(gg[1], wg[1], 1e-5, rel=True, what="grad_bg")
        assert not mask.requires_grad
        assert torch.equal(mask, WF.grid_sample(torch.ones(frames * no, 1, ho, wo, device=dev), gobj))
    want, wg = spelled((0.5, 0.5), 0.0)
    got, gg, _ = fused((0.5, 0.5), 0.0)
    close(got, want, 1e-6, what="out, (x + 1) / 2 folded into the taps")
    for a, bb, name in zip(gg, wg, ("grad_obj", "grad_bg", "grad_grid_obj", "grad_grid_bg")):
        close(a, bb, 1e-5, rel=True, what=name)
    # the CPU restatement of the spelled-out form
    leaves = [x.detach().cpu().requires_grad_() for x in (obj, bg, gobj, gbg)]
    o, g, go, gb = leaves
    if shared:
        oe = o.view(b, 1, no, c, ho, wo).expand(-1, t, -1, -1, -1, -1).reshape(frames * no, c, ho, wo)
        ge = g.view(b, 1, c, h, w).expand(-1, t, -1, -1, -1).reshape(frames, c, h, w)
    else:
        oe, ge = o, g
    ref = torch.cat([O.grid_sample_delta((ge + 1) / 2, gb, 0.0).view(frames, 1, c, h, w),
                     O.grid_sample_delta((oe + 1) / 2, go, 0.0).view(frames, no, c, h, w)], dim=1)
    (ref * wgt.cpu()).sum().backward()
    close(got, ref, what="out vs oracle")
    for a, x, name in zip(gg, leaves, ("grad_obj", "grad_bg", "grad_grid_obj", "grad_grid_bg")):
        close(a, x.grad, rel=True, what=name + " vs oracle")
    with pytest.raises(_lib.WaldoHipError):
        WF.layers_to_output(obj, bg, gobj[:-1], gbg)          # not a whole number of objects per frame
    with pytest.raises(_lib.WaldoHipError):
        WF.layers_to_output(obj, bg[:, :1], gobj, gbg)        # channel counts differ
    empty = WF.layers_to_output(obj[:0], bg if shared else bg, gobj[:0], gbg, 0.0, 0.0, None, bbc)
    assert empty.shape == (frames, 1, c, h, w)                 # no objects: the background alone
    assert torch.equal(empty[:, 0], WF.grid_sample(bg, gbg, delta=0.0, broadcast=bbc))


def test_grid_sample_empty(dev):
    from waldo_amd import functional as WF
    out = WF.grid_sample(torch.zeros(0, 3, 4, 4, device=dev), torch.zeros(0, 5, 5, 2, device=dev))
    assert out.shape == (0, 3, 5, 5)


# ----------------------------------------------------------------------------- A6
@pytest.mark.parametrize("nl", [1, 2, 5, 8, 9, 12, 17, 21, 32])
def test_occ_composite(dev, nl):
    from waldo_amd import functional as WF
    torch.manual_seed(nl)
    m, h, w, div = 6, 9, 31, 3
    alpha = torch.rand(m, nl, h, w, requires_grad=True)
    occ = torch.rand(m // div, nl, nl, requires_grad=True)
    occ_full = occ.repeat_interleave(div, dim=0)
    ref = O.occlusion_product(alpha, occ_full)
    wgt = torch.randn(ref.shape)
    (ref * wgt).sum().backward()
    a2, o2 = alpha.detach().to(dev).requires_grad_(), occ.detach().to(dev).requires_grad_()
    out = WF.occ_composite(a2, o2, occ_div=div)
    close(out, ref, what="out")
    (out * wgt.to(dev)).sum().backward()
    close(a2.grad, alpha.grad, rel=True, what="grad_alpha")
    close(o2.grad, occ.grad, rel=True, what="grad_occ")


def test_occ_composite_golden(dev, golden):
    from waldo_amd import functional as WF
    g = golden("occ_comp")
    v = (g["vid"] + 1) / 2
    alpha = v[:, :, :, -1].clone()
    alpha[:, :, 0] = 1.0
    b, t, nl, h, w = alpha.shape
    out = WF.occ_composite(alpha.view(b * t, nl, h, w).to(dev), g["occ"].view(b * t, nl, nl).to(dev))
    close(out.view(b, t, nl, h, w) * 2 - 1, g["alpha"], what="alpha")


# ----------------------------------------------------------------------------- fused path
def _oracle_fused(layers, pts, occ, ctrl, w1, w2, dtype, loss="weights", delta=0.0):
    """Oracle outputs and autograd gradients in `dtype` from the same fp32 inputs/buffers."""
    f, nl, _, h, w = layers.shape
    inv, rep = O.tps_init(h, w, ctrl)
    l = layers.detach().to(dtype).requires_grad_()
    p = pts.detach().to(dtype).requires_grad_()
    o = occ.detach().to(dtype).requires_grad_()
    rgb, alpha = O.warp_composite(l, p, o, inv.to(dtype), rep.to(dtype), delta=delta)
    if loss == "weights":
        ((rgb * w1.to(dtype)).sum() + (alpha * w2.to(dtype)).sum()).backward()
    else:
        rgb.square().mean().backward()
    return rgb.detach(), alpha.detach(), l.grad, p.grad, o.grad


def _hip_fused(dev, layers, pts, occ, ctrl, w1, w2, loss="weights", buffers=None, generic=False, delta=0.0):
    from waldo_amd import functional as WF
    import waldo_amd
    from waldo_amd import _lib
    # 0: tiled backward where it applies (L <= 17, K3 == 19); 1: the generic kernel for every shape
    assert _lib.load().waldo_set_debug_option(_lib.DEBUG_BWD_GENERIC, int(generic)) == 0
    f, nl, _, h, w = layers.shape
    tps = waldo_amd.TPSWarp(h, w, ctrl)
    if buffers is not None:  # as when a reference checkpoint is loaded
        tps.load_state_dict(buffers, strict=False)
    tps = tps.to(dev)
    l2 = layers.detach().to(dev).requires_grad_()
    p2 = pts.detach().to(dev).requires_grad_()
    o2 = occ.detach().to(dev).requires_grad_()
    try:
        rgb, alpha = WF.warp_composite(l2, p2, o2, tps.inverse_kernel, tps.basis_t, return_alpha=True, delta=delta)
        if loss == "weights":
            ((rgb * w1.to(dev)).sum() + (alpha * w2.to(dev)).sum()).backward()
        else:
            rgb.square().mean().backward()
    finally:
        _lib.load().waldo_set_debug_option(_lib.DEBUG_BWD_GENERIC, 0)  # must not leak into other tests
    return rgb, alpha, l2.grad, p2.grad, o2.grad


def _matched(dev, layers, pts, occ, ctrl, w1, w2, loss="weights", delta=0.0):
    """The oracle at the fused path's OWN sample coordinates (oracle/wif_oracle.py:warp_composite_px), in fp32 and
    fp64: every floor and in-range decision is the kernel's, so the control-point gradient -- discontinuous where a
    sample crosses a texel boundary -- is compared at plain TOL * scale, and every other output per element.  The
    coordinates are the fmaf chain of tps_eval() (warp_composite_kernels.hip.h) over the device's own mapping,
    reproduced on the host (oracle/c_oracle.py); the same chain without the pixel scaling must give WF.tps_grid's
    output bit for bit, on every call, and the coordinates must be within the fp32 error bound of the two chains
    (mapping and grid: 2 (N + K3) 2^-24 sum|terms|, in fp64) of the oracle's own fp64 ones."""
    from oracle import c_oracle
    from waldo_amd import functional as WF
    import waldo_amd
    f, nl, _, h, w = layers.shape
    tps = waldo_amd.TPSWarp(h, w, ctrl).to(dev)
    with torch.no_grad():
        pd = pts.detach().to(dev)
        mapping = WF.tps_mapping(tps.inverse_kernel, pd).cpu()
        grid = WF.tps_grid(tps.inverse_kernel, tps.basis_t, pd, h, w).cpu()
    basis = tps.basis_t.cpu()
    plain = torch.from_numpy(c_oracle.tps_chain(basis, mapping, h, w, scaled=False)).view(grid.shape)
    assert torch.equal(plain.view(torch.int32), grid.view(torch.int32)), \
        f"host fmaf chain != WF.tps_grid in {int((plain != grid).sum())} of {grid.numel()} coordinates"
    pos = torch.from_numpy(c_oracle.tps_chain(basis, mapping, h, w, scaled=True)).view(f * nl, h, w, 2)
    inv, rep = O.tps_init(h, w, ctrl)
    size = torch.tensor([w, h], dtype=torch.float64)
    pos64 = ((O.tps_grid(inv.double(), rep.double(), pts.double(), h, w) + 1) * size - 1) / 2
    k3, n = basis.shape[0], pts.shape[1]
    x = torch.cat([pts.double(), pts.new_zeros(pts.shape[0], 3, 2, dtype=torch.float64)], dim=1).abs()
    m_abs = mapping.double().abs() + inv.double().abs() @ x                    # |m_k| + sum_n |inv_kn x_n|
    terms = (basis.double().t().abs() @ (m_abs * size / 2)).view(f * nl, h, w, 2)
    slack = (pos.double() - pos64).abs() - 2 * (n + k3) * 2.0 ** -24 * (terms + size)
    assert slack.max() <= 0, f"coordinates off the fp64 TPS chain by up to {slack.max().item():.3e} px"
    out = []
    for dt in (torch.float32, torch.float64):
        l, p, o = (x.detach().to(dt).requires_grad_() for x in (layers, pts, occ))
        rgb, alpha = O.warp_composite_px(l, p, o, inv.to(dt), rep.to(dt), pos, delta=delta)
        if loss == "weights":
            ((rgb * w1.to(dt)).sum() + (alpha * w2.to(dt)).sum()).backward()
        else:
            rgb.square().mean().backward()
        out.append((rgb.detach(), alpha.detach(), l.grad, p.grad, o.grad))
    return out


def _compare_fused(hip, m32, m64):
    compare_warp_composite(hip, m32, m64)


@pytest.mark.parametrize("tag", ["small", "l8", "big_warp"])
def test_warp_composite_golden(dev, golden, tag):
    """HIP vs the REFERENCE's own outputs/gradients (golden vectors)."""
    g = golden(f"warp_composite_{tag}")
    f, nl, _, h, w = g["layers"].shape
    inv, rep = O.tps_init(h, w, g["ctrl"])
    ref64 = _oracle_fused(g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"], torch.float64)
    hip = _hip_fused(dev, g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"])
    # d loss / d score through compute_occ, chained on the CPU from the kernel's d loss / d occ
    score = g["score"].clone().requires_grad_()
    O.compute_occ(score)[:, 0].backward(hip[4].cpu())
    s64 = g["score"].double().requires_grad_()
    O.compute_occ(s64)[:, 0].backward(ref64[4])
    # against the reference's own outputs where they are continuous in the sample positions ...
    for i, name in enumerate(("rgb", "alpha", "grad_layers")):
        close(hip[i], g[name], rel=i >= 2, what=name + " vs the reference", exact=ref64[i])
    # ... its control-point gradient, taken at ITS sample positions, at the bound it always had (the tensor's largest
    # fp32 noise: a sample the reference rounds across a texel boundary moves every entry of that map) ...
    close(hip[3], g["grad_pts"], rel=True, what="grad_pts vs the reference", exact=ref64[3], noise_of="tensor")
    # ... and everything against the oracle at the kernel's coordinates
    _compare_fused(hip, *_matched(dev, g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"]))
    close(score.grad, g["grad_score"], rel=True, what="grad_score", exact=s64.grad)


@pytest.mark.parametrize("tag", ["delta1", "delta1_big", "delta_half"])
def test_warp_composite_delta_golden(dev, golden, tag):
    """The "-delta" padding of Warper.obj_to_output / bg_to_output (lvd.py:548,559) on the fused path
    vs the REFERENCE's F.grid_sample(x + delta) - delta -> reduce_comp (outputs and autograd)."""
    g = golden(f"warp_composite_{tag}")
    delta = float(g["delta"])
    ref64 = _oracle_fused(g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"], torch.float64, delta=delta)
    hip = _hip_fused(dev, g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"], delta=delta)
    for i, name in enumerate(("rgb", "alpha", "grad_layers")):
        close(hip[i], g[name], rel=i >= 2, what=name + " vs the reference", exact=ref64[i])
    close(hip[3], g["grad_pts"], rel=True, what="grad_pts vs the reference", exact=ref64[3], noise_of="tensor")
    _compare_fused(hip, *_matched(dev, g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"], delta=delta))
    # and the padding matters here: delta = 0 gives another picture
    plain = _hip_fused(dev, g["layers"], g["pts"], g["occ"], g["ctrl"], g["w1"], g["w2"])
    assert (plain[0].cpu() - g["rgb"]).abs().max() > 1e-2


@pytest.mark.parametrize("cfg", [
    dict(f=2, nl=8, h=64, w=96, sigma=0.15), dict(f=2, nl=8, h=32, w=48, sigma=0.6),   # staged; boxes too large
    dict(f=2, nl=5, h=17, w=33, sigma=0.2), dict(f=1, nl=17, h=32, w=64, sigma=0.2),     # plain forward; LP = 17
    dict(f=2, nl=8, h=32, w=48, sigma=0.2, generic=True), dict(f=1, nl=24, h=16, w=32, sigma=0.2),
])
def test_warp_composite_delta_random(dev, cfg):
    """delta = 1 through every kernel variant (LDS-staged border path, oversize-box fallback, plain
    forward, two-kernel and generic backward) against the oracle in fp32 and fp64."""
    f, nl, h, w = cfg["f"], cfg["nl"], cfg["h"], cfg["w"]
    ctrl = O.get_grid(4, 4).view(-1, 2)
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=nl + 50, sigma=cfg["sigma"])
    torch.manual_seed(f * 10 + nl)
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    hip = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2, generic=cfg.get("generic", False), delta=1.0)
    _compare_fused(hip, *_matched(dev, layers, pts, occ, ctrl, w1, w2, delta=1.0))


def test_warp_composite_golden_bench_loss(dev, golden):
    """The benchmark's loss (rgb.square().mean()) and the rgb-only output path."""
    from waldo_amd import functional as WF
    import waldo_amd
    g = golden("warp_composite_l8")
    f, nl, _, h, w = g["layers"].shape
    ref64 = _oracle_fused(g["layers"], g["pts"], g["occ"], g["ctrl"], None, None, torch.float64, "sq")
    tps = waldo_amd.TPSWarp(h, w, g["ctrl"]).to(dev)
    l2 = g["layers"].to(dev).requires_grad_()
    p2 = g["pts"].to(dev).requires_grad_()
    rgb = WF.warp_composite(l2, p2, g["occ"].to(dev), tps.inverse_kernel, tps.basis_t)
    close(rgb, g["rgb"], what="rgb", exact=ref64[0])
    rgb.square().mean().backward()
    close(l2.grad, g["grad_layers_sq"], rel=True, what="grad_layers", exact=ref64[2])
    close(p2.grad, g["grad_pts_sq"], rel=True, what="grad_pts vs the reference", exact=ref64[3], noise_of="tensor")
    m32, m64 = _matched(dev, g["layers"], g["pts"], g["occ"], g["ctrl"], None, None, "sq")
    _compare_fused((rgb, None, l2.grad, p2.grad, None), m32, m64)


@pytest.mark.parametrize("cfg", [
    dict(f=1, nl=1, h=5, w=7), dict(f=2, nl=2, h=16, w=16), dict(f=3, nl=4, h=17, w=33),
    dict(f=2, nl=5, h=24, w=40), dict(f=5, nl=8, h=32, w=48), dict(f=2, nl=9, h=20, w=20),
    dict(f=2, nl=12, h=16, w=24), dict(f=1, nl=17, h=16, w=32), dict(f=1, nl=20, h=12, w=12),
    dict(f=1, nl=32, h=8, w=16), dict(f=2, nl=8, h=16, w=16, k=3), dict(f=2, nl=3, h=16, w=16, k=5),
    dict(f=40, nl=4, h=16, w=16), dict(f=2, nl=8, h=64, w=96, smooth=8),
    dict(f=2, nl=17, h=32, w=64, smooth=4), dict(f=3, nl=8, h=40, w=56, sigma=0.6),
    dict(f=1, nl=3, h=96, w=256, sigma=0.3), dict(f=2, nl=8, h=64, w=128, smooth=4),
    dict(f=2, nl=6, h=72, w=192, sigma=0.02, smooth=4), dict(f=2, nl=8, h=32, w=48, generic=True),
    dict(f=2, nl=4, h=17, w=33, generic=True),
])
def test_warp_composite_random(dev, cfg):
    """Seeded random cases: every padded-L variant, ragged sizes (H*W not a multiple of the
    workgroup), other control-point counts (generic K3 path), smooth layers (strict 1e-4 bound),
    violent warps (sigma=0.3-0.6: folds, samples out of range, bounding boxes too large for the
    LDS image, more than 24 intersecting tiles) and the generic backward kernel."""
    f, nl, h, w = cfg["f"], cfg["nl"], cfg["h"], cfg["w"]
    k = cfg.get("k", 4)
    ctrl = O.get_grid(k, k).view(-1, 2)
    if nl == 1:
        torch.manual_seed(1)
        layers = torch.rand(f, 1, 4, h, w) * 2 - 1
        pts = ctrl.view(1, -1, 2) + 0.1 * torch.randn(f, k * k, 2)
        occ = torch.zeros(f, 1, 1)
    else:
        layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, k_side=k, seed=nl,
                                                  sigma=cfg.get("sigma", 0.1),
                                                  smooth=cfg.get("smooth", 0))
    torch.manual_seed(f * 100 + nl)
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    hip = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2, generic=cfg.get("generic", False))
    _compare_fused(hip, *_matched(dev, layers, pts, occ, ctrl, w1, w2))


def test_warp_composite_seeded_fuzz(dev):
    """Twenty-four shapes drawn from a seeded generator -- 1 ... 5 frames, 1 ... 32 layers, rasters of 4 ... 64 by
    4 ... 110 pixels (any remainder against the 16 x 16 / 4 x 64 / 32 x 64 tiles and the four-pixel vectors), 3 x 3 ...
    5 x 5 control points, mild to folding warps, the three `delta` paddings, both backward kernels -- forward and all
    three gradients against the fp32 and fp64 oracle at the kernel's own coordinates through the same
    `_compare_fused` as every other case, the control-point gradient on every draw.  The fixed lists
    above hold the shapes somebody thought of; this holds the ones nobody did."""
    import random
    rng = random.Random(20260)
    for case in range(24):
        f, nl = rng.randint(1, 5), rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 18, 23, 24, 25, 31, 32])
        h, w = rng.randint(4, 64), rng.randint(4, 110)
        if nl > 17:  # (the oracle's L^2 product in fp64: keep the big layer counts small)
            f, h, w = min(f, 2), min(h, 40), min(w, 72)
        k = rng.choice([3, 4, 4, 4, 5])
        sigma = rng.choice([0.05, 0.1, 0.2, 0.35, 0.5])
        delta = rng.choice([0.0, 0.0, 0.5, 1.0])
        generic = rng.random() < 0.25
        smooth = rng.choice([0, 2, 4])
        ctrl = O.get_grid(k, k).view(-1, 2)
        if nl == 1:
            torch.manual_seed(case)
            layers = torch.rand(f, 1, 4, h, w) * 2 - 1
            pts = ctrl.view(1, -1, 2) + sigma * torch.randn(f, k * k, 2)
            occ = torch.zeros(f, 1, 1)
        else:
            layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, k_side=k, seed=1000 + case, sigma=sigma,
                                                      smooth=smooth)
        torch.manual_seed(case)
        w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
        hip = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2, generic=generic, delta=delta)
        try:
            # grad_pts on every draw, white-noise layers included: the fp64 oracle takes each sample where the kernel
            # does, so a texel boundary that one fp32 evaluation rounds to the other side is no longer a difference
            _compare_fused(hip, *_matched(dev, layers, pts, occ, ctrl, w1, w2, delta=delta))
        except AssertionError as exc:
            raise AssertionError(f"case {case}: f={f} nl={nl} h={h} w={w} k={k} sigma={sigma} delta={delta} "
                                 f"generic={generic} smooth={smooth}: {exc}") from exc


def test_warp_composite_smooth_is_strict(dev):
    """On smooth layers the fp32 reference is itself determined to ~1e-6, so the bound that is
    enforced is the plain north-star 1e-4 (checked here without the noise allowance)."""
    f, nl, h, w = 2, 8, 128, 128
    ctrl = O.get_grid(4, 4).view(-1, 2)
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=21, smooth=8)
    torch.manual_seed(0)
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    ref32 = _oracle_fused(layers, pts, occ, ctrl, w1, w2, torch.float32)
    hip = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2)
    close(hip[0], ref32[0], what="rgb")
    close(hip[1], ref32[1], what="alpha")
    close(hip[2], ref32[2], rel=True, what="grad_layers")
    close(hip[3], ref32[3], tol=1e-3, rel=True, what="grad_pts")
    close(hip[4], ref32[4], tol=1e-3, rel=True, what="grad_occ")


def test_warp_composite_empty(dev):
    from waldo_amd import functional as WF
    import waldo_amd
    tps = waldo_amd.TPSWarp(8, 8, O.get_grid(4, 4).view(-1, 2)).to(dev)
    rgb = WF.warp_composite(torch.zeros(0, 3, 4, 8, 8, device=dev), torch.zeros(0, 16, 2, device=dev),
                            torch.zeros(0, 3, 3, device=dev), tps.inverse_kernel, tps.basis_t)
    assert rgb.shape == (0, 3, 8, 8)


def test_warp_composite_rejects_bad_shapes(dev):
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    import waldo_amd
    tps = waldo_amd.TPSWarp(8, 8, O.get_grid(4, 4).view(-1, 2)).to(dev)
    with pytest.raises(WaldoHipError):
        WF.warp_composite(torch.zeros(1, 33, 4, 8, 8, device=dev), torch.zeros(33, 16, 2, device=dev),
                          torch.zeros(1, 33, 33, device=dev), tps.inverse_kernel, tps.basis_t)


# ----------------------------------------------------------------------------- full size
@pytest.mark.parametrize("h,w,nl,smooth", [(128, 128, 8, 0), (256, 512, 8, 0), (256, 512, 8, 8)])
def test_warp_composite_full_size(dev, h, w, nl, smooth):
    """BASELINE.json sizes: (i) oracle (fp32 and fp64) on the same seeded inputs for a few
    frames, fwd+bwd with the benchmark's loss; (ii) size-independent properties: identity control
    points => plain composite of the unwarped layers; transparent objects => layer 0's rgb."""
    from waldo_amd import functional as WF
    import waldo_amd
    f = 2
    layers, pts, occ, inv, rep = O.make_synthetic(f, nl, h, w, seed=11, smooth=smooth)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    hip = _hip_fused(dev, layers, pts, occ, ctrl, None, None, "sq")
    _compare_fused(hip[:4] + (None,), *_matched(dev, layers, pts, occ, ctrl, None, None, "sq"))
    # (ii) identity control points and (iii) transparent objects: against the oracle first ...
    tps = waldo_amd.TPSWarp(h, w, ctrl).to(dev)
    ld, od = layers.to(dev), occ.to(dev)
    ident = ctrl.view(1, 16, 2).expand(f * nl, -1, -1).contiguous()
    rgb_i = WF.warp_composite(ld, ident.to(dev), od, tps.inverse_kernel, tps.basis_t)
    id64 = _oracle_fused(layers, ident, occ, ctrl, None, None, torch.float64, "sq")[0]
    id32 = _oracle_fused(layers, ident, occ, ctrl, None, None, torch.float32, "sq")[0]
    close(rgb_i, id32, what="identity warp vs oracle", exact=id64, noise_of="tensor")
    l0 = layers.clone()
    l0[:, 1:, 3] = -1.0
    rgb_0 = WF.warp_composite(l0.to(dev), ident.to(dev), od, tps.inverse_kernel, tps.basis_t)
    bg64 = _oracle_fused(l0, ident, occ, ctrl, None, None, torch.float64, "sq")[0]
    bg32 = _oracle_fused(l0, ident, occ, ctrl, None, None, torch.float32, "sq")[0]
    close(rgb_0, bg32, what="background only vs oracle", exact=bg64, noise_of="tensor")
    # ... then the size-independent properties themselves.  They hold only approximately, for the
    # reference as for the build: the TPS fixed point is reached to ~3e-6 in grid units (1e-3 px
    # at W=512), and at the image border that leaks a little zero padding into the sample.
    if smooth:
        plain, _, _ = O.reduce_comp(layers.unsqueeze(1), occ.unsqueeze(1))
        close(rgb_i, plain[:, 0], tol=2e-2, what="identity warp = plain composite")
        close(rgb_0, layers[:, 0, :3], tol=2e-2, what="transparent objects = layer 0")


def test_c3_eight_frames_with_grad_occ(dev):
    """BASELINE config C3 (256x512, L = 8, fwd+bwd with the benchmark's loss) on 8 frames, with
    occ.requires_grad (the GOCC variant of the pixel kernel): every output and gradient, grad_occ
    included, against the fp32 and fp64 oracle on the same seeded inputs."""
    f, nl, h, w = 8, 8, 256, 512
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=13)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    hip = _hip_fused(dev, layers, pts, occ, ctrl, None, None, "sq")
    _compare_fused(hip, *_matched(dev, layers, pts, occ, ctrl, None, None, "sq"))


@pytest.mark.parametrize("name,f,nl,h,w,bwd", [
    ("C4 KITTI 256x832 L=8", 2, 8, 256, 832, True),
    ("C5 Cityscapes 512x1024 L=12", 2, 12, 512, 1024, True),
    ("recipe L=17 512x1024", 1, 17, 512, 1024, True),
])
def test_baseline_configs_on_hip(dev, name, f, nl, h, w, bwd):
    """BASELINE.json configs C4 / C5 and the recipe's L = 17 (scripts/cityscapes/train_wif.sh:12-14)
    at full raster size on the HIP path, a couple of frames each, against the fp32 and fp64 oracle;
    L = 12 and L = 17 go through the two-kernel backward (the workspace query must say so)."""
    from waldo_amd import _lib
    assert _lib.load().waldo_warp_composite_bwd_workspace_bytes(f, nl, h, w, 19) > 0, name
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=nl + w)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    hip = _hip_fused(dev, layers, pts, occ, ctrl, None, None, "sq")
    _compare_fused(hip, *_matched(dev, layers, pts, occ, ctrl, None, None, "sq"))


@pytest.mark.parametrize("nl", [12, 17])
def test_two_kernel_backward_equals_generic(dev, nl):
    """L = 12 / 17 (C5, the recipe): the two-kernel backward against the generic per-tap-atomics
    kernel on the same inputs -- same records, different accumulation (fixed point vs float atomics)."""
    f, h, w = 2, 64, 96
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=nl, smooth=4)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    torch.manual_seed(nl)
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    tiled = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2)
    generic = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2, generic=True)
    assert torch.equal(tiled[0], generic[0]) and torch.equal(tiled[1], generic[1])
    for i, name in ((2, "grad_layers"), (3, "grad_pts"), (4, "grad_occ")):
        close(tiled[i], generic[i], tol=2e-5, rel=True, what=name)


@pytest.mark.parametrize("nl", [8, 17, 24, 32])
def test_staged_forward_equals_plain_forward(dev, nl):
    """The LDS-staged forward (MFMA grid, footprint boxes in LDS) against the plain gather forward,
    bit for bit, for every padded layer count -- the guard for the L >= 24 variants, which are only
    correct while hipcc keeps their MFMA accumulators out of AGPRs (warp_composite_fwd_lds.hip.h)."""
    from waldo_amd import _lib, functional as WF
    import waldo_amd
    f, h, w = 2, 64, 128
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=nl + 1)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    args = (layers.to(dev), pts.to(dev), occ.to(dev), tps.inverse_kernel, tps.basis_t)
    lib = _lib.load()
    with torch.no_grad():
        staged = WF.warp_composite(*args, return_alpha=True)
        assert lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 1) == 0
        try:
            plain = WF.warp_composite(*args, return_alpha=True)
        finally:
            lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 0)
    assert torch.equal(staged[0], plain[0]) and torch.equal(staged[1], plain[1])


@pytest.mark.parametrize("where", ["grad_rgb", "layers"])
def test_non_finite_gradients_stay_visible(dev, where):
    """A NaN in the incoming gradient or in a layer must reach grad_layers on BOTH backward paths
    (the reference's training loop checks its gradients for NaN): the generic kernel propagates
    it per texel, the two-kernel path turns every source tile the poisoned cell reaches into NaN."""
    from waldo_amd import _lib, functional as WF
    import waldo_amd
    f, nl, h, w = 2, 8, 64, 96
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=4, smooth=4)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    wgt = torch.ones(f, 3, h, w)
    if where == "grad_rgb":
        wgt[1, 2, 40, 50] = float("nan")
    else:
        layers[0, 3, 1, 20, 30] = float("nan")
    out = {}
    for generic in (False, True):
        assert _lib.load().waldo_set_debug_option(_lib.DEBUG_BWD_GENERIC, int(generic)) == 0
        try:
            ld = layers.to(dev).requires_grad_()
            rgb = WF.warp_composite(ld, pts.to(dev), occ.to(dev), tps.inverse_kernel, tps.basis_t)
            (rgb * wgt.to(dev)).sum().backward()
            out[generic] = ld.grad
        finally:
            _lib.load().waldo_set_debug_option(_lib.DEBUG_BWD_GENERIC, 0)
    fr = 1 if where == "grad_rgb" else 0
    for generic, g in out.items():
        assert torch.isnan(g[fr]).any(), f"generic={generic}: the NaN disappeared"
        assert torch.isfinite(g[1 - fr]).all(), f"generic={generic}: the other frame must stay finite"


def test_fixed_point_precision_inside_a_tile(dev):
    """Dynamic range inside one 32x64 source tile of the two-kernel backward: the alpha plane's
    gradient is made 1000x larger than the colour planes' (separate scales: the colour planes must
    keep their precision), and half of the tile's pixels carry a 1e-3x smaller incoming gradient.
    Per texel against the generic kernel (float atomics, fp32 relative precision): the documented
    ABSOLUTE bound per channel group, 2^-12 of the group's largest magnitude -- observed errors are
    orders of magnitude below -- and, since round 3, scales per 8x16 SUB-BLOCK: the texels of the
    small half that no large contribution can reach keep 1e-4-level RELATIVE precision (with one
    scale per tile they had percent-level: ADVICE round 2); the test pins include/waldo_hip.h."""
    f, nl, h, w = 1, 4, 32, 64
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=8, smooth=4, sigma=0.03)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    w1 = torch.ones(f, 3, h, w)
    w1[..., : w // 2] *= 1e-3
    w2 = 1000.0 * torch.ones(f, nl, h, w)
    tiled = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2)
    generic = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2, generic=True)
    gt, gg = tiled[2].double().cpu(), generic[2].double().cpu()
    for name, sl in (("colour", slice(0, 3)), ("alpha", slice(3, 4))):
        err = (gt[:, :, sl] - gg[:, :, sl]).abs().max().item()
        mag = gg[:, :, sl].abs().max().item()
        print(f"[fixed point] {name}: max err {err:.3e}, max |grad| {mag:.3e}, ratio {err / mag:.2e}")
        assert err <= mag * 2.0 ** -12, (name, err, mag)
    # the small half of the colour planes: its own magnitude is 1e-3 of the tile's colour maximum and
    # 3e-6 of the alpha plane's; the quantum of the colour group (~1e-5 of ITS maximum) leaves it
    # percent-level relative precision -- a scale shared with the alpha plane would have flushed it
    # to zero
    small = gg[:, :, :3, :, 4: w // 2 - 8]
    err_small = (gt[:, :, :3, :, 4: w // 2 - 8] - small).abs().max().item()
    print(f"[fixed point] small half: max err {err_small:.3e}, max |grad| {small.abs().max().item():.3e}")
    assert err_small <= 5e-2 * small.abs().max().item(), (err_small, small.abs().max().item())
    # the first sub-block column (texels 0 .. 15): no footprint box of the large half reaches it (the
    # warp moves a pixel by about one texel here), so its quantum follows ITS OWN bound
    own = gg[:, :, :3, :, 2:14]
    err_own = (gt[:, :, :3, :, 2:14] - own).abs().max().item()
    print(f"[fixed point] sub-blocks of the small half: max err {err_own:.3e}, max |grad| {own.abs().max().item():.3e}")
    assert err_own <= 2e-4 * own.abs().max().item(), (err_own, own.abs().max().item())


@pytest.mark.parametrize("shape", [(2, 8, 64, 96), (3, 5, 40, 72)])
def test_warp_composite_vs_c_oracle(dev, shape):
    """HIP path vs the plain-C restatement (oracle/wif_oracle.c: double precision, its own TPS
    buffers) on smooth layers -- an oracle that shares no code, no library and no buffer with the
    product; the north-star 1e-4 on the outputs, 1e-3 relative on the gradients (the product's fp32
    K^-1 buffer alone moves them by ~1e-4)."""
    from oracle import c_oracle as C
    f, nl, h, w = shape
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=17, smooth=8)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    torch.manual_seed(2)
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    ref = C.fused(layers.numpy(), pts.numpy(), occ.numpy(), ctrl.numpy(), w1.numpy(), w2.numpy())
    hip = _hip_fused(dev, layers, pts, occ, ctrl, w1, w2)
    close(hip[0], torch.from_numpy(ref["rgb"]), what="rgb")
    close(hip[1], torch.from_numpy(ref["alpha"]), what="alpha")
    close(hip[2], torch.from_numpy(ref["grad_layers"]), tol=1e-3, rel=True, what="grad_layers")
    close(hip[3], torch.from_numpy(ref["grad_pts"]), tol=1e-3, rel=True, what="grad_pts")
    close(hip[4], torch.from_numpy(ref["grad_occ"]), tol=1e-3, rel=True, what="grad_occ")


def test_backward_reproducible_and_linear(dev):
    """Size-independent properties at the benchmark shape (256x512, L = 8, 16 frames): the layer and
    control-point gradients are BITWISE identical from run to run (no float atomics on that path:
    source-tile ownership, fixed-point LDS sums, fixed-order partial reduction), and the backward is
    linear in the incoming gradient (2x the loss => 2x every gradient, exactly: the fixed-point scale
    is a power of two that follows the bound)."""
    from waldo_amd import functional as WF
    import waldo_amd
    f, nl, h, w = 16, 8, 256, 512
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=5)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    od = occ.to(dev)
    torch.manual_seed(3)
    wgt = torch.randn(f, 3, h, w, device=dev)

    def grads(scale):
        ld, pd = layers.to(dev).requires_grad_(), pts.to(dev).requires_grad_()
        rgb = WF.warp_composite(ld, pd, od, tps.inverse_kernel, tps.basis_t)
        (rgb * wgt).sum().mul(scale).backward()
        return rgb.detach(), ld.grad, pd.grad

    r1, gl1, gp1 = grads(1.0)
    r2, gl2, gp2 = grads(1.0)
    assert torch.equal(r1, r2) and torch.equal(gl1, gl2) and torch.equal(gp1, gp2)
    _, gl3, gp3 = grads(2.0)
    assert torch.equal(gl3, 2 * gl1)
    close(gp3, 2 * gp1, tol=1e-6, rel=True, what="grad_pts linear")
    assert torch.isfinite(gl1).all() and gl1.abs().sum() > 0


def test_long_batches_go_in_pieces(dev, monkeypatch):
    """More frames than one launch / one workspace takes: the wrapper splits along the (independent)
    frames; outputs and gradients equal the single call bit for bit."""
    from waldo_amd import functional as WF
    import waldo_amd
    f, nl, h, w = 7, 4, 16, 32
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=9)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)

    def run():
        ld, pd = layers.to(dev).requires_grad_(), pts.to(dev).requires_grad_()
        rgb, alpha = WF.warp_composite(ld, pd, occ.to(dev), tps.inverse_kernel, tps.basis_t, return_alpha=True)
        (rgb.square().mean() + alpha.mean()).backward()
        return rgb.detach(), alpha.detach(), ld.grad, pd.grad

    whole = run()
    monkeypatch.setattr(WF, "MAX_FL_PER_LAUNCH", 3 * nl)       # 3 frames per call
    assert WF._frames_per_call(f, nl, h, w, 19) == 3
    pieces = run()
    for a, b in zip(whole, pieces):
        assert torch.equal(a, b)
    monkeypatch.setattr(WF, "MAX_FL_PER_LAUNCH", 65535)
    monkeypatch.setattr(WF, "MAX_WORKSPACE_BYTES", 2 * WF._lib.load().waldo_warp_composite_bwd_workspace_bytes(1, nl, h, w, 19))
    assert 1 <= WF._frames_per_call(f, nl, h, w, 19) <= 3


@pytest.mark.parametrize("f,nl", [(2, 8), (6, 5), (12, 4)])
def test_short_batches_use_every_xcd_and_change_no_bit(dev, f, nl):
    """Batches whose frame-chunk count is not a multiple of the 8 XCDs cut every frame's tiles into
    bands (waldo_common.hip.h:xcd_decode_banded; 4 / 4 / 2 bands here); frames are independent, so
    the batch must equal its frames computed one call at a time (8 bands each), bit for bit --
    forward, layer gradients (two-kernel backward) and control-point gradients."""
    from waldo_amd import functional as WF
    import waldo_amd
    h, w = 96, 160
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=21)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    torch.manual_seed(4)
    wgt = torch.randn(f, 3, h, w, device=dev)

    def run(sl):
        ld = layers[sl].to(dev).requires_grad_()
        pd = pts.view(f, nl, 16, 2)[sl].reshape(-1, 16, 2).to(dev).requires_grad_()
        rgb = WF.warp_composite(ld, pd, occ[sl].to(dev), tps.inverse_kernel, tps.basis_t)
        (rgb * wgt[sl]).sum().backward()
        return rgb.detach(), ld.grad, pd.grad.view(-1, nl, 16, 2)

    whole = run(slice(0, f))
    for i in range(f):
        one = run(slice(i, i + 1))
        for a, b in zip(whole, one):
            assert torch.equal(a[i:i + 1], b), i


def test_batches_beyond_four_gibibytes_change_no_bit(dev):
    """A batch whose layer stack, gradient and record workspace each pass 4 GiB (300 frames of the headline shape:
    5.0 GB of layers) -- 2.7 x the headline's 112 frames: every offset inside the fused forward and the two-kernel
    backward that is kept in 32 bits must be an offset inside a plane or a frame, not inside the batch.  Frames are
    independent: the first, a middle and the last three frames of the batch equal the same frames computed as a batch
    of their own, bit for bit (forward, layer and control-point gradients), and the whole result is finite."""
    from waldo_amd import functional as WF
    import waldo_amd
    f, nl, h, w = 300, 8, 256, 512
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    g = torch.Generator(device=dev).manual_seed(9)
    layers = torch.rand(f, nl, 4, h, w, device=dev, generator=g) * 2 - 1
    assert layers.numel() * 4 > 4 * 2 ** 30
    pts = O.get_grid(4, 4).view(1, 16, 2).to(dev) + 0.05 * torch.randn(f * nl, 16, 2, device=dev, generator=g)
    occ = O.compute_occ(torch.randn(f, 1, nl - 1, generator=torch.Generator().manual_seed(9)))[:, 0].to(dev)

    wgt = torch.randn(f, 3, h, w, device=dev, generator=g)

    def run(idx):
        ld = layers[idx].clone().requires_grad_()
        pd = pts.view(f, nl, 16, 2)[idx].reshape(-1, 16, 2).clone().requires_grad_()
        rgb = WF.warp_composite(ld, pd, occ[idx], tps.inverse_kernel, tps.basis_t)
        (rgb * wgt[idx]).sum().backward()
        return rgb.detach(), ld.grad, pd.grad.view(-1, nl, 16, 2)

    whole = run(torch.arange(f, device=dev))
    for t in whole:
        assert torch.isfinite(t).all()
    probe = torch.tensor([0, 149, 297, 298, 299], device=dev)
    part = run(probe)
    for name, a, b in zip(("rgb", "grad_layers", "grad_pts"), whole, part):
        assert torch.equal(a[probe], b), name
    del whole, part, layers, wgt
    torch.cuda.empty_cache()


@pytest.mark.parametrize("f,nl,h,w,delta", [(8, 8, 128, 128, 0.0), (3, 5, 40, 72, 1.0), (1, 12, 64, 96, 0.0),
                                            (5, 17, 32, 64, 0.5)])
def test_forward_from_control_points_is_one_launch_and_the_same_bits(dev, f, nl, h, w, delta):
    """Without autograd the forward goes straight from the control points
    (waldo_warp_composite_pts_fwd: the TPS mapping of warp.py:52-53 computed inside the kernel, a
    frame ahead); rgb and the composited alphas must carry the same bits as tps_mapping + the
    two-step forward that runs under autograd."""
    from waldo_amd import functional as WF
    import waldo_amd
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=31)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    ld, pd, od = layers.to(dev), pts.to(dev), occ.to(dev)
    assert WF._lib.load().waldo_warp_composite_pts_supported(nl, h, w, 16)
    assert f * ((h + 15) // 16) * ((w + 15) // 16) <= WF.FOLD_MAX_TILE_FRAMES  # the folded path is taken
    with torch.no_grad():
        rgb1, a1 = WF.warp_composite(ld, pd, od, tps.inverse_kernel, tps.basis_t, return_alpha=True, delta=delta)
    rgb2, a2 = WF.warp_composite(ld, pd.clone().requires_grad_(), od, tps.inverse_kernel, tps.basis_t,
                                 return_alpha=True, delta=delta)
    assert torch.equal(rgb1, rgb2.detach()) and torch.equal(a1, a2.detach())
    inv, rep = tps.inverse_kernel.cpu(), tps.tgt_grid_repr.cpu()
    ref, ref_a = O.warp_composite(layers, pts, occ, inv, rep, delta=delta)
    e64, e64_a = O.warp_composite(layers.double(), pts.double(), occ.double(), inv.double(), rep.double(), delta=delta)
    close(rgb1, ref, what="rgb (control-point forward)", exact=e64)
    close(a1, ref_a, what="alpha (control-point forward)", exact=e64_a)


def test_graphed_forward_replay(dev):
    """A captured HIP graph of the fused forward replays bit-identically on new input contents
    (the library launches on the capturing stream and never synchronises)."""
    from waldo_amd import functional as WF
    from waldo_amd.graphs import GraphedCall
    import waldo_amd
    f, nl, h, w = 4, 8, 32, 64
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)

    def fwd(layers, pts, occ):
        return WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)

    a = [x.to(dev) for x in O.make_synthetic(f, nl, h, w, seed=1)[:3]]
    b = [x.to(dev) for x in O.make_synthetic(f, nl, h, w, seed=2, sigma=0.2)[:3]]
    g = GraphedCall(fwd, *a)
    with torch.no_grad():
        for inp in (a, b, a):
            assert torch.equal(g(*inp), fwd(*inp))
    with pytest.raises(ValueError):
        g(a[0][:1], a[1], a[2])


def test_small_ops_seeded_fuzz(dev):
    """The single-op entry points over shapes from a seeded generator, each against the oracle's expression of the
    same op, forward and backward: ``grid_sample`` (any input / output raster, samples up to 20 % outside the image,
    the three deltas), ``occ_composite`` (1 ... 32 layers, shared occlusion matrices), ``wif_fuse`` (1 ... 6 contexts,
    5 ... 40 channels, with and without the sigmoid term).  24 cases each."""
    import random
    from oracle import warper_oracle as WO
    from waldo_amd import functional as WF
    rng = random.Random(99)
    for case in range(24):
        torch.manual_seed(case)
        # --- grid_sample
        n, c = rng.randint(1, 6), rng.randint(1, 40)
        hi, wi, ho, wo = rng.randint(1, 70), rng.randint(1, 140), rng.randint(1, 70), rng.randint(1, 140)
        delta = rng.choice([0.0, 0.5, 1.0])
        x = torch.randn(n, c, hi, wi, requires_grad=True)
        grid = (torch.rand(n, ho, wo, 2) * 2.4 - 1.2).requires_grad_()
        ref = O.grid_sample_delta(x, grid, delta)
        wgt = torch.randn(ref.shape)
        (ref * wgt).sum().backward()
        x2, g2 = x.detach().to(dev).requires_grad_(), grid.detach().to(dev).requires_grad_()
        out = WF.grid_sample(x2, g2, delta=delta)
        (out * wgt.to(dev)).sum().backward()
        tag = f"case {case} grid_sample {n}x{c}x{hi}x{wi} -> {ho}x{wo} delta {delta}"
        close(out, ref, what=tag + " out")
        close(x2.grad, x.grad, rel=True, what=tag + " grad_x")
        close(g2.grad, grid.grad, rel=True, what=tag + " grad_grid")
        # --- occ_composite
        nl, div = rng.choice([1, 2, 3, 5, 8, 9, 12, 13, 17, 18, 24, 31, 32]), rng.randint(1, 3)
        m, h, w = div * rng.randint(1, 3), rng.randint(1, 40), rng.randint(1, 90)
        alpha = torch.rand(m, nl, h, w, requires_grad=True)
        occ = torch.rand(m // div, nl, nl, requires_grad=True)
        ref = O.occlusion_product(alpha, occ.repeat_interleave(div, dim=0))
        wgt = torch.randn(ref.shape)
        (ref * wgt).sum().backward()
        a2, o2 = alpha.detach().to(dev).requires_grad_(), occ.detach().to(dev).requires_grad_()
        out = WF.occ_composite(a2, o2, occ_div=div)
        (out * wgt.to(dev)).sum().backward()
        tag = f"case {case} occ_composite m={m} nl={nl} {h}x{w} div={div}"
        close(out, ref, what=tag + " out")
        close(a2.grad, alpha.grad, rel=True, what=tag + " grad_alpha")
        close(o2.grad, occ.grad, rel=True, what=tag + " grad_occ")
        # --- wif_fuse
        b, t, tc, cv, co = rng.randint(1, 2), rng.randint(1, 3), rng.randint(1, 6), rng.randint(5, 40), rng.choice([4, 5])
        h, w, ab = rng.randint(1, 50), rng.randint(1, 130), rng.random() < 0.7
        vid = torch.randn(b, t, tc, cv, h, w, requires_grad=True)
        net = torch.randn(b, t, tc, co, h, w, requires_grad=True)
        ref = WO.wif_fuse(vid, net, ab=ab)
        wgt = torch.randn(ref.shape)
        (ref * wgt).sum().backward()
        v2, n2 = vid.detach().to(dev).requires_grad_(), net.detach().to(dev).requires_grad_()
        out = WF.wif_fuse(v2, n2, ab=ab)
        (out * wgt.to(dev)).sum().backward()
        tag = f"case {case} wif_fuse b={b} t={t} tc={tc} c={cv} co={co} {h}x{w} ab={ab}"
        close(out, ref, what=tag + " out")
        close(v2.grad, vid.grad, rel=True, what=tag + " grad_vid")
        close(n2.grad, net.grad, rel=True, what=tag + " grad_net")
