"""GPU: the single-op kernels on the operands their paths depend on (tests/regimes.py) -- occ_composite and compute_occ
on sparse layered alphas and planted occlusion scores, wif_fuse / wif_fuse_bytes on a wide gate and unbounded softmax
logits (a masked context, two equal maxima), the grid_sample family on maps that take the wave-uniform early exits,
make runs of equal texel addresses, hit texel centres and boundaries exactly, and on inputs of one or two texels a
side.  Every comparison is tests/parity.py:close at the project's TOL, the fp32 oracle as the reference and the fp64
oracle as `exact` (the criteria of regimes.py, which tests/test_operand_regimes_cpu.py runs on the oracle alone); each
test first asserts on the host that its operands take the path it is named after.

Measured on an MI355X, the worst comparison of each kernel (pytest -s prints every one):
  nl=32 occ_composite out: |hip-ref32| 0.000e+00  |hip-ref64| 3.588e-07  |ref32-ref64| 3.588e-07  worst 0.00374 x its bound
  nl=32 occ_composite grad_alpha: |hip-ref32| 1.192e-06  |hip-ref64| 1.245e-06  |ref32-ref64| 1.189e-06  worst 0.00302 x
  No=31 compute_occ grad_score: |hip-ref32| 2.697e-06  |hip-ref64| 9.318e-07  |ref32-ref64| 2.762e-06  worst 0.00515 x
  (2, 1, 4, 40, 5, 8, 16) ab=True wif_fuse out: |hip-ref32| 2.384e-07  |hip-ref64| 4.408e-07  |ref32-ref64| 3.516e-07  worst 0.00439 x
  (1, 1, 1, 5, 4, 9, 13) ab=True wif_fuse grad_net: |hip-ref32| 4.768e-07  |hip-ref64| 4.768e-07  |ref32-ref64| 0  worst 0.14 x
    (one context: the score's true gradient is 0, the channel's scale the floor of 1e-2 of the tensor's)
  (5, 1) four-pixel form grid_sample out: |hip-ref32| 5.364e-07  |hip-ref64| 9.153e-07  |ref32-ref64| 8.109e-07  worst 0.00908 x
  constant delta=0.5 grid_sample grad_grid: |hip-ref32| 1.073e-06  |hip-ref64| 1.009e-05  |ref32-ref64| 9.374e-06  worst 0.00612 x
  (5, 1) one-pixel form grid_sample grad_x: |hip-ref32| 5.960e-07  |hip-ref64| 1.606e-06  |ref32-ref64| 1.606e-06  worst 0.00485 x
  layers_to_output grad_obj: |hip-ref32| 1.192e-06  |hip-ref64| 7.530e-07  |ref32-ref64| 8.724e-07  worst 0.00285 x"""
import pytest
import torch

import regimes as R
from oracle import wif_oracle as O
from parity import close

pytestmark = pytest.mark.gpu

HALF = (torch.bfloat16, torch.float16)


def _leaves(dev, *tensors):
    return [x.detach().to(dev).requires_grad_() for x in tensors]


# ------------------------------------------------------------------------------------------ occ_composite / compute_occ
@pytest.mark.parametrize("nl", R.OCC_LAYERS)
def test_occ_composite_on_sparse_alphas(dev, nl):
    from waldo_amd import functional as WF
    alpha, occ, wgt, ref32, ref64 = R.occ_case(nl)
    assert ref32[0].amax(dim=(0, 2, 3)).min() >= 0.1            # every layer is there to be judged
    a, o = _leaves(dev, alpha, occ)
    out = WF.occ_composite(a, o, occ_div=alpha.shape[0] // occ.shape[0])
    (out * wgt.to(dev)).sum().backward()
    R.check_occ((out, a.grad, o.grad), ref32, ref64, tag=f"nl={nl} ")
    # the pixel column of exact zeros stays exactly zero (the column of exact ones is judged with the rest)
    assert (alpha[..., 0] == 0).all() and (alpha[..., 1] == 1).all() and (out[..., 0] == 0).all()


@pytest.mark.parametrize("no", [16, 31])
def test_compute_occ_on_planted_scores(dev, no):
    from waldo_amd import functional as WF
    score, wgt, ref32, ref64 = R.score_case(no)
    assert all((score == v).any() for v in R.PLANTED_SCORES)
    (s,) = _leaves(dev, score)
    occ = WF.compute_occ(s)
    (occ * wgt.to(dev)).sum().backward()
    R.check_scores((occ, s.grad), ref32, ref64, tag=f"No={no} ")
    # exact ties: 0.5 off the diagonal, 0 on it, wherever the oracle has them
    tie = ref32[0] == 0.5
    assert tie.sum() >= 2 * score.shape[0] and (occ.cpu()[tie] == 0.5).all()
    assert (occ.cpu()[:, 0].diagonal(dim1=1, dim2=2) == 0).all()


# ------------------------------------------------------------------------------------------ wif_fuse
def _wif_asserts(shape, vid, net):
    gate = torch.sigmoid(vid[:, :, :, 4] + 5)
    assert gate.min() < 1e-3 and gate.max() > 0.999
    if shape[2] >= 2:
        assert net[:, :, :, 3].max() > 89 and (net[:, :, 0, 3, R.MASKED_ROW] == float("-inf")).all()


@pytest.mark.parametrize("ab", [True, False])
@pytest.mark.parametrize("shape", R.WIF_SHAPES)
def test_wif_fuse_on_a_wide_gate_and_unbounded_logits(dev, shape, ab):
    from waldo_amd import functional as WF
    vid, net, wgt, ref32, ref64 = R.wif_case(shape, ab)
    _wif_asserts(shape, vid, net)
    v, n = _leaves(dev, vid, net)
    out = WF.wif_fuse(v, n, ab=ab)
    (out * wgt.to(dev)).sum().backward()
    assert torch.isfinite(out).all() and torch.isfinite(v.grad).all() and torch.isfinite(n.grad).all()
    R.check_wif((out, v.grad, n.grad), ref32, ref64, tag=f"{shape} ab={ab} ")
    if shape[2] >= 2:  # a masked context gets no gradient at all
        assert (n.grad[:, :, 0, :, R.MASKED_ROW] == 0).all()
        assert (ref32[2][:, :, 0, :, R.MASKED_ROW] == 0).all()


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", R.WIF_SHAPES)
def test_wif_fuse_bytes_on_the_regime(dev, shape, layout):
    from waldo_amd import functional as WF
    for ab in (True, False):
        vid, net = (x.to(dev) for x in R.wif_case(shape, ab)[:2])
        fp32 = WF.wif_fuse(vid, net, ab=ab)
        for q in ("trunc", "round"):
            got = WF.wif_fuse_bytes(vid, net, ab=ab, quantize=q, layout=layout)
            want = WF.frames_to_bytes(fp32, quantize=q, layout=layout)
            assert got.dtype == torch.uint8 and got.shape == want.shape
            assert torch.equal(got, want), (ab, q)
        # (values clipped at both ends, and values between)
        assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()


@pytest.mark.parametrize("ndt", [torch.float32, *HALF])
@pytest.mark.parametrize("vdt", [torch.float32, *HALF])
def test_wif_fuse_dtype_pairs_on_the_regime(dev, vdt, ndt):
    """As test_gpu_half.py:test_wif_fuse_dtype_pairs asserts on randn: the 16-bit (vid, net) pairs equal the call on
    the widened fp32 tensors, the forward bit for bit, the gradients rounded to their inputs' types."""
    from test_gpu_half import same_rounded
    from waldo_amd import functional as WF
    shape = R.WIF_SHAPES[0]
    vid32, net32, wgt = R.wif_case(shape, True)[:3]
    vid, net = vid32.to(dev).to(vdt).requires_grad_(), net32.to(dev).to(ndt).requires_grad_()
    _wif_asserts(shape, vid.detach().float().cpu(), net.detach().float().cpu())
    v32, n32 = vid.detach().float().requires_grad_(), net.detach().float().requires_grad_()
    out, ref = WF.wif_fuse(vid, net), WF.wif_fuse(v32, n32)
    assert out.dtype == torch.float32 and torch.equal(out, ref) and torch.isfinite(out).all()
    out.backward(wgt.to(dev))
    ref.backward(wgt.to(dev))
    assert vid.grad.dtype == vdt and net.grad.dtype == ndt
    assert same_rounded(vid.grad, v32.grad) if vdt != torch.float32 else torch.equal(vid.grad, v32.grad)
    assert same_rounded(net.grad, n32.grad) if ndt != torch.float32 else torch.equal(net.grad, n32.grad)


# ------------------------------------------------------------------------------------------ grid_sample
def _assert_path(name, grid):
    """The path the map is named after, from the grid itself."""
    hi, wi = R.GS_INPUT[2:]
    runs = R.address_runs(grid, hi, wi)
    if name == "affine":
        assert grid.shape[1] * grid.shape[2] % 1024 == 0                     # whole wavefronts of the 4-pixel forward
        assert R.spans_all_outside(grid, hi, wi, 256) >= 1 and R.spans_straddling(grid, hi, wi, 256) >= 1
        assert R.spans_all_outside(grid, hi, wi, 64) >= 1
        assert (runs >= 4).any() and runs.max() == 16
    elif name == "constant":
        assert R.any_tap_valid(grid, hi, wi).all() and runs.min() >= 4 and runs.max() == 16
    else:
        assert grid.shape[1] * grid.shape[2] % 4 == 0 and (grid.abs() >= 1e29).any()
        ix = ((grid + 1.0) * 8.0 - 1.0) * 0.5
        assert (ix % 1 == 0).any() and (ix % 1 == 0.5).any()


def _hip_grid_sample(dev, x, grid, wgt, delta, det=False):
    import waldo_amd
    from waldo_amd import functional as WF
    xi, gr = _leaves(dev, x, grid)
    with waldo_amd.deterministic(det):
        out = WF.grid_sample(xi, gr, delta=delta)
        (out * wgt.to(dev)).sum().backward()
    return out.detach(), xi.grad, gr.grad


@pytest.mark.parametrize("delta", R.GS_DELTAS)
@pytest.mark.parametrize("name", R.GS_MAPS)
def test_grid_sample_on_structured_maps(dev, name, delta):
    x, grid, wgt, ref32, ref64 = R.gs_case(name, delta)
    _assert_path(name, grid)
    got = _hip_grid_sample(dev, x, grid, wgt, delta)
    R.check_gs(got, ref32, ref64, tag=f"{name} delta={delta} ")
    # zero padding is exact: a pixel without a tap inside the input (the wild coordinates among them) is -delta, and
    # its coordinates get no gradient
    outside = ~R.any_tap_valid(grid, *R.GS_INPUT[2:])
    if name == "dyadic":
        wild = (grid.abs() >= 1e29).any(dim=-1)
        assert wild.any() and (outside | ~wild).all()
    if outside.any():
        picked = got[0].cpu().movedim(1, -1)[outside]
        assert (picked == -delta).all() and (ref32[0].movedim(1, -1)[outside] == -delta).all()
        assert (got[2].cpu()[outside] == 0).all()


@pytest.mark.parametrize("delta", R.GS_DELTAS)
@pytest.mark.parametrize("name", R.GS_MAPS)
def test_grid_sample_deterministic_on_structured_maps(dev, name, delta):
    x, grid, wgt, ref32, ref64 = R.gs_case(name, delta)
    _assert_path(name, grid)
    atomic = _hip_grid_sample(dev, x, grid, wgt, delta)
    det = _hip_grid_sample(dev, x, grid, wgt, delta, det=True)
    assert torch.equal(det[0], atomic[0]) and torch.equal(det[2], atomic[2])
    R.check_gs(det, ref32, ref64, tag=f"deterministic {name} delta={delta} ")


@pytest.mark.parametrize("name", R.GS_MAPS)
def test_grid_sample_mask_on_structured_maps(dev, name):
    from waldo_amd import functional as WF
    x, grid = (t.to(dev) for t in R.gs_case(name, 0.0)[:2])
    _assert_path(name, grid.cpu())
    ones = torch.ones(x.shape[0], 1, *x.shape[2:], device=dev)
    with torch.no_grad():
        for delta in R.GS_DELTAS:
            out, mask = WF.grid_sample(x, grid, delta=delta, return_mask=True)
            assert torch.equal(out, WF.grid_sample(x, grid, delta=delta))
            assert torch.equal(mask, WF.grid_sample(ones, grid, delta=0.0))
    outside = ~R.any_tap_valid(grid.cpu(), *R.GS_INPUT[2:])
    assert (mask.cpu()[:, 0][outside] == 0).all()


def test_layers_to_output_on_the_affine_map(dev):
    """WF.layers_to_output with pre = (0.5, 0.5) -- `(x + 1) / 2` folded into the taps -- against the spelled-out
    oracle, on grids whose first and last wavefronts have every tap outside: there the output is -delta whatever the
    pre-affine."""
    from waldo_amd import functional as WF
    frames, no, c, delta = 2, 2, 3, 1.0
    hi, wi = R.GS_INPUT[2:]
    g = torch.Generator().manual_seed(900)
    obj, bg = torch.randn(frames * no, c, hi, wi, generator=g), torch.randn(frames, c, hi, wi, generator=g)
    gobj, gbg = R.affine_map(32, 64, frames * no), R.affine_map(32, 64, frames)
    _assert_path("affine", gobj)
    h, w = gbg.shape[1:3]
    wgt = torch.randn(frames, no + 1, c, h, w, generator=g)

    def run(dt):
        o, b, go, gb = (x.detach().to(dt, copy=True).requires_grad_() for x in (obj, bg, gobj, gbg))
        out = torch.cat([O.grid_sample_delta((b + 1) / 2, gb, delta).view(frames, 1, c, h, w),
                         O.grid_sample_delta((o + 1) / 2, go, delta).view(frames, no, c, h, w)], dim=1)
        (out * wgt.to(dt)).sum().backward()
        return out.detach(), o.grad, b.grad, go.grad, gb.grad

    ref32, ref64 = run(torch.float32), run(torch.float64)
    o, b, go, gb = _leaves(dev, obj, bg, gobj, gbg)
    out = WF.layers_to_output(o, b, go, gb, delta, delta, None, None, (0.5, 0.5))
    (out * wgt.to(dev)).sum().backward()
    got = (out, o.grad, b.grad, go.grad, gb.grad)
    names = ("out", "grad_obj", "grad_bg", "grad_grid_obj", "grad_grid_bg")
    for i, name in enumerate(names):
        close(got[i], ref32[i], rel=i > 0, what="layers_to_output " + name, exact=ref64[i])
    outside = ~R.any_tap_valid(gbg, hi, wi)
    assert (out.detach().cpu().movedim(2, -1)[:, 0][outside] == -delta).all()


@pytest.mark.parametrize("hw", R.DEGENERATE_INPUTS)
def test_grid_sample_on_inputs_of_one_or_two_texels(dev, hw):
    """Hi, Wi of 1 and 2: `pairs == false` of the four-pixel forward (Wi = 1), and the pair origin pinned to column 0
    with shift in {-1, 0, +1} on every sample (Wi = 2).  The four-pixel form (8 x 8) and the one-pixel form (7 x 9)
    against the oracle, and against each other bit for bit on the 56 sample points both grids hold."""
    delta = 0.5
    x, wgt8, wgt9, grid8, grid9, refs8, refs9 = R.degenerate_case(*hw, delta)
    assert grid8.shape[1] * grid8.shape[2] % 4 == 0 and grid9.shape[1] * grid9.shape[2] % 4 != 0
    assert torch.equal(grid9[:, :, :8], grid8[:, :7])
    if hw[1] == 2:
        assert R.pair_shifts(grid8, *hw).unique().tolist() == [-1, 0, 1]
    got8 = _hip_grid_sample(dev, x, grid8, wgt8, delta)
    got9 = _hip_grid_sample(dev, x, grid9, wgt9, delta)
    R.check_gs(got8, *refs8, tag=f"{hw} four-pixel form ")
    R.check_gs(got9, *refs9, tag=f"{hw} one-pixel form ")
    assert torch.equal(got8[0][:, :, :7], got9[0][:, :, :, :8])
