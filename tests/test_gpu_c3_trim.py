"""The training step's trimmed work, on the smallest shapes where its paths can go wrong.

Two things left the C3 step without changing a value ("C3 trim"):
  * layer 0's alpha plane is not loaded by the staged forward or by K1: reduce_comp replaces the background's alpha
    by 1 (oracle/wif_oracle.py: reduce_comp), so no output and no gradient depends on that plane;
  * the staged forward takes 16 x 32 tiles for 5 .. 8 fp32 layers once the launch has 2048 of them, else 16 x 16.
The control-point gradient's contract is pinned with them (a third trim, its reduce inside K2's launch, was measured
and not kept): summed in a fixed order, and ADDED to the caller's buffer.

Shapes: F = 3, L = 8 and L = 3 (a padded-L instance), K3 = 19, at 40 x 72 and 16 x 36 -- partial 16 x 16, 16 x 32 and
32 x 64 tiles, 4 | W, more than one K2 tile per plane at 40 x 72 -- with delta 0 and 1 and a control-point noise of
0.15 (boxes cross the border) and 0.6 (folds: boxes too large for the staged image, the gather fallback).  Every
comparison against the oracle goes through tests/parity.py, at its tolerances."""
import functools

import pytest
import torch

from oracle import wif_oracle as O

pytestmark = pytest.mark.gpu

CASES = [(nl, h, w, delta, sigma) for nl in (8, 3) for h, w in ((40, 72), (16, 36)) for delta in (0.0, 1.0)
         for sigma in (0.15, 0.6)]


@functools.lru_cache(maxsize=None)
def _case(nl, h, w, delta, sigma):
    """Inputs, loss weights and the oracle at the kernels' own coordinates (fp32 and fp64): computed once, read only."""
    import test_gpu_parity as tp
    dev = torch.device("cuda:0")
    f = 3
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=7 * nl + h, sigma=sigma)
    torch.manual_seed(nl * 1000 + h)
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    ctrl = O.get_grid(4, 4).view(-1, 2)
    m32, m64 = tp._matched(dev, layers, pts, occ, ctrl, w1, w2, delta=delta)
    return layers, pts, occ, ctrl, w1, w2, m32, m64


def _abi_operands(dev, layers, pts, occ, ctrl):
    import waldo_amd
    from waldo_amd import functional as WF
    h, w = layers.shape[-2:]
    tps = waldo_amd.TPSWarp(h, w, ctrl).to(dev)
    with torch.no_grad():
        mapping = WF.tps_mapping(tps.inverse_kernel, pts.to(dev)).contiguous()
    return layers.to(dev).contiguous(), tps.basis_t.contiguous(), mapping, occ.to(dev).contiguous(), tps


def _abi_backward(dev, layers, basis_t, mapping, occ, grad_rgb, grad_alpha, delta, gm):
    """waldo_warp_composite_bwd through the C ABI on the two-kernel path: grad_layers (written), gm (added to)."""
    from waldo_amd import _lib
    f, nl, _, h, w = layers.shape
    k3 = mapping.shape[1]
    nbytes = _lib.query("waldo_warp_composite_bwd_workspace_bytes", f, nl, h, w, k3)
    assert nbytes > 0, "these shapes are the two-kernel backward's"
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    gl = torch.full_like(layers, float("nan"))  # every texel is written
    _lib.launch("waldo_warp_composite_bwd", dev, layers, basis_t, mapping, occ, grad_rgb, grad_alpha, gl, gm, None, ws,
                nbytes, f, nl, h, w, k3, float(delta))
    return gl


def _same_forward(got, plain, delta, what):
    """A staged forward against the plain one: bit for bit at delta == 0 (tests/test_gpu_parity.py:
    test_staged_forward_equals_plain_forward).  With a delta the plain kernel -- and the staged kernels' gather of a
    layer whose box does not fit their image -- shift every tap by it and back, the staged sampling only the taps of
    pixels near the border (in the interior the weights sum to 1 and the shift cancels -- in exact arithmetic), so the
    two differ by the rounding of (x + delta) - delta, 2.4e-7 here, before this change as after it: the project's
    forward tolerance then."""
    from parity import close
    for g, p, name in zip(got, plain, ("rgb", "alpha")):
        if delta == 0:
            assert torch.equal(g, p), f"{what}: {name} differs from the plain forward"
        else:
            close(g, p, what=f"{what}: {name} vs the plain forward, delta {delta}")


def _staged_and_plain(args, delta):
    from waldo_amd import _lib, functional as WF
    lib = _lib.load()
    with torch.no_grad():
        staged = WF.warp_composite(*args, return_alpha=True, delta=delta)
        assert lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 1) == 0
        try:
            plain = WF.warp_composite(*args, return_alpha=True, delta=delta)
        finally:
            lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 0)
    return staged, plain


@pytest.mark.parametrize("nl,h,w,delta,sigma", CASES)
def test_trimmed_step_keeps_its_values(dev, nl, h, w, delta, sigma):
    import test_gpu_parity as tp
    layers, pts, occ, ctrl, w1, w2, m32, m64 = _case(nl, h, w, delta, sigma)
    f = layers.shape[0]
    # the staged forward against the plain one, bit for bit (16 x 16 tiles: the launch is far below the rule's bar)
    ld, basis_t, mapping, od, tps = _abi_operands(dev, layers, pts, occ, ctrl)
    staged, plain = _staged_and_plain((ld, pts.to(dev), od, tps.inverse_kernel, tps.basis_t), delta)
    _same_forward(staged, plain, delta, "one-launch forward")
    # the backward against the fp32 and fp64 oracle, the project's comparison and tolerances
    hip = tp._hip_fused(dev, layers, pts, occ, ctrl, w1, w2, delta=delta)
    tp._compare_fused(hip, m32, m64)
    _same_forward(hip[:2], plain, delta, "two-step forward")  # (as training runs it)
    assert torch.equal(hip[0], staged[0]) and torch.equal(hip[1], staged[1])
    # twice: the same bits (grad_occ is summed with float atomics outside deterministic mode: not part of this)
    again = tp._hip_fused(dev, layers, pts, occ, ctrl, w1, w2, delta=delta)
    assert torch.equal(hip[2], again[2]), "grad_layers differs between two runs"
    assert torch.equal(hip[3], again[3]), "grad_pts differs between two runs"
    # grad_mapping through the C ABI: reproducible, and ADDED to what the buffer holds
    w1d, w2d = w1.to(dev), w2.to(dev)
    gm1, gm2 = torch.zeros_like(mapping), torch.zeros_like(mapping)
    gl1 = _abi_backward(dev, ld, basis_t, mapping, od, w1d, w2d, delta, gm1)
    gl2 = _abi_backward(dev, ld, basis_t, mapping, od, w1d, w2d, delta, gm2)
    assert torch.equal(gm1, gm2) and torch.equal(gl1, gl2) and torch.equal(gl1, hip[2])
    assert gm1.abs().max() > 0
    torch.manual_seed(5)
    before = torch.randn(mapping.shape).to(dev)
    gm3 = before.clone()
    _abi_backward(dev, ld, basis_t, mapping, od, w1d, w2d, delta, gm3)
    assert torch.equal(gm3, before + gm1), "grad_mapping is not accumulated into the caller's buffer"
    assert f * nl == mapping.shape[0]


@pytest.mark.parametrize("with_grad_alpha", [False, True])
@pytest.mark.parametrize("nl,h,w,delta,sigma", [c for c in CASES if c[4] == 0.6 or c[1] == 40])
def test_layer0_alpha_plane_does_not_matter(dev, nl, h, w, delta, sigma, with_grad_alpha):
    """The same call with layer 0's alpha plane replaced by other finite values: every output and gradient has the
    same bits, and the plane's own gradient is zero.  (Finite values only: a NaN there reaches the grid gradient through
    0 x NaN in the reference as well.)"""
    import test_gpu_parity as tp
    layers, pts, occ, ctrl, w1, w2, _, _ = _case(nl, h, w, delta, sigma)
    other = layers.clone()
    other[:, 0, 3] = -0.75
    other[:, 0, 3, ::3, 1::2] = 0.5
    if with_grad_alpha:
        a, b = (tp._hip_fused(dev, x, pts, occ, ctrl, w1, w2, delta=delta) for x in (layers, other))
    else:
        a, b = (tp._hip_fused(dev, x, pts, occ, ctrl, None, None, "sq", delta=delta) for x in (layers, other))
    for i, name in enumerate(("rgb", "alpha", "grad_layers", "grad_pts")):
        assert torch.equal(a[i], b[i]), f"{name} depends on layer 0's alpha plane"
    for g in (a[2], b[2]):
        assert (g[:, 0, 3] == 0).all(), "grad_layers[:, 0, 3] must be zero"
    # grad_mapping itself, and the plain forward
    for x in (layers, other):
        ld, basis_t, mapping, od, tps = _abi_operands(dev, x, pts, occ, ctrl)
        gm = torch.zeros_like(mapping)
        _abi_backward(dev, ld, basis_t, mapping, od, w1.to(dev), w2.to(dev) if with_grad_alpha else None, delta, gm)
        staged, plain = _staged_and_plain((ld, pts.to(dev), od, tps.inverse_kernel, tps.basis_t), delta)
        if x is layers:
            gm_a, staged_a = gm, staged
        else:
            assert torch.equal(gm, gm_a), "grad_mapping depends on layer 0's alpha plane"
            assert torch.equal(staged[0], staged_a[0]) and torch.equal(staged[1], staged_a[1])
        _same_forward(staged, plain, delta, "one-launch forward")


@pytest.mark.parametrize("nl", [8, 6])
def test_both_tile_forms_equal_the_plain_forward(dev, nl):
    """Shapes on either side of the launcher's rule (warp_composite_kernels.hip.h: fwd_wide_tiles): 17 frames of
    200 x 328 are 17 x 143 = 2431 tiles of 16 x 32 -- over the bar of 2048, so the 16 x 32 form runs, with partial tiles on
    both edges -- and the first 3 of those frames alone run the 16 x 16 form.  The two forms against each other and
    against the plain forward (_same_forward); L = 6 is the padded instance."""
    import waldo_amd
    from waldo_amd import _lib, functional as WF
    h, w, f = 200, 328, 17
    g = torch.Generator(device=dev).manual_seed(nl)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    layers = torch.rand(f, nl, 4, h, w, generator=g, device=dev) * 2 - 1
    pts = O.get_grid(4, 4).view(1, 16, 2).to(dev) + 0.15 * torch.randn(f * nl, 16, 2, generator=g, device=dev)
    occ = O.compute_occ(torch.randn(f, 1, nl - 1, generator=g, device=dev).cpu())[:, 0].to(dev)
    layers.requires_grad_()  # (a call that wants gradients takes the two-step forward, as training does)
    lib = _lib.load()

    def forward(n, delta):
        return WF.warp_composite(layers[:n], pts[:n * nl], occ[:n], tps.inverse_kernel, tps.basis_t, return_alpha=True,
                                 delta=delta)

    for delta in (0.0, 1.0):
        wide, narrow = forward(f, delta), forward(3, delta)
        assert lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 1) == 0
        try:
            plain = forward(f, delta)
        finally:
            lib.waldo_set_debug_option(_lib.DEBUG_FWD_PLAIN, 0)
        # (a layer whose box fits one tile form's image and not the other's is gathered the plain kernel's way)
        _same_forward((wide[0][:3], wide[1][:3]), narrow, delta, "16 x 32 against 16 x 16 tiles")
        _same_forward(wide, plain, delta, "16 x 32 tiles")
