"""The operand regimes of tests/regimes.py on the CPU, from the oracle alone (in the manner of
test_parity_sensitivity.py): the regimes hold -- each builder makes the operands its kernel path depends on, and the fp32 oracle passes the GPU
tests' own criteria on them --, the operands of the existing single-op tests do not hold them (stated as assertions, so
that the reason for tests/test_gpu_regimes.py stays visible), and the new criteria reject restatements with one planted
error that the old operands or bounds accept."""
import pytest
import torch

import regimes as R
from oracle import warper_oracle as WO
from oracle import wif_oracle as O
from parity import TOL, close


def _clone(ref):
    return [x.clone() for x in ref]


# ------------------------------------------------------------------------------------------ the regimes hold
@pytest.mark.parametrize("nl", R.OCC_LAYERS)
def test_sparse_alphas_keep_every_layer_visible(nl):
    alpha, occ, _, ref32, ref64 = R.occ_case(nl)
    assert alpha.min() == 0 and alpha.max() == 1
    assert (alpha[..., 0] == 0).all() and (alpha[..., 1] == 1).all()
    per_pixel = (alpha[..., 2:] >= 0.3).sum(dim=1)
    assert (per_pixel == min(3, nl)).all()
    out = ref32[0]
    per_layer = out.amax(dim=(0, 2, 3))
    share = (out > 1e-2).float().mean(dim=(0, 2, 3))
    print(f"[regime] nl={nl}: smallest layer maximum {per_layer.min().item():.3f}, smallest share above 1e-2 "
          f"{share.min().item():.3f}")
    assert per_layer.min() >= 0.1
    assert share.min() >= 0.05
    if nl >= 12:  # (nl - 1 scores hold the planted pair and all nine planted values)
        off = ~torch.eye(nl, dtype=torch.bool)
        assert ((occ == 0.5) & off).any() and (occ[:, 1:, 1:][:, off[1:, 1:]] < 1e-5).any() and (occ > 1 - 1e-5).any()
    # the fp32 oracle passes the GPU test's criterion, and is within TOL of its fp64 self without the noise allowance
    R.check_occ(ref32, ref32, ref64)
    close(ref32[0], ref64[0], rel=True, what="fp32 vs fp64 out", slice_dims=(1,))
    close(ref32[1], ref64[1], rel=True, what="fp32 vs fp64 grad_alpha")
    close(ref32[2], ref64[2], rel=True, what="fp32 vs fp64 grad_occ")


@pytest.mark.parametrize("no", [16, 31])
def test_planted_scores_reach_the_tails_and_the_ties(no):
    score, _, ref32, ref64 = R.score_case(no)
    for row in score[:, 0]:
        for v in R.PLANTED_SCORES:
            assert (row == v).any()
        assert row.unique().numel() < no  # two equal scores
    occ = ref32[0][:, 0, 1:, 1:]
    off = ~torch.eye(no, dtype=torch.bool)
    assert (occ[:, off] == 0.5).sum() >= 2 * score.shape[0]
    assert (occ.diagonal(dim1=1, dim2=2) == 0).all()
    assert all(torch.isfinite(t).all() for t in ref32 + ref64)
    assert ref32[1].abs().max() > 0
    R.check_scores(ref32, ref32, ref64)
    close(ref32[0], ref64[0], what="fp32 vs fp64 occ")
    close(ref32[1], ref64[1], rel=True, what="fp32 vs fp64 grad_score")


def test_affine_map_takes_the_wave_uniform_paths():
    grid = R.gs_map("affine")
    n, hi, wi = grid.shape[0], *R.GS_INPUT[2:]
    assert R.spans_all_outside(grid, hi, wi, 256) == 2 * n   # the early exit of the four-pixel forward
    assert R.spans_straddling(grid, hi, wi, 256) >= 1        # ... and wavefronts that must not take it
    assert R.spans_all_outside(grid, hi, wi, 64) == 8 * n    # `scatter == false` of the backward
    runs = R.address_runs(grid, hi, wi)
    print(f"[regime] affine map: longest run {int(runs.max())}, mean {runs.float().mean().item():.2f} lanes")
    assert (runs >= 4).any() and runs.max() == 16
    # (its un-normalised coordinates keep their distance from every integer: one floor in fp32 and fp64)
    ix = ((grid.double() + 1) * 8 - 1) / 2
    assert ((ix - ix.round()).abs() >= 1 / 32).all()


def test_constant_and_dyadic_maps():
    hi, wi = R.GS_INPUT[2:]
    grid = R.gs_map("constant")
    runs = R.address_runs(grid, hi, wi)
    assert R.any_tap_valid(grid, hi, wi).all() and runs.max() == 16 and runs.min() >= 4
    x0, y0 = R.corners(grid, hi, wi)
    assert (0 <= x0).all() and (x0 < wi - 1).all() and (0 <= y0).all() and (y0 < hi - 1).all()  # an interior point
    grid = R.gs_map("dyadic")
    assert grid.shape[1] * grid.shape[2] % 4 == 0
    ix = ((grid.double() + 1) * 8 - 1) / 2
    ix32 = ((grid + 1.0) * 8.0 - 1.0) * 0.5
    assert torch.equal(ix32.double(), ix)                    # exact in fp32
    inside = (ix[..., 0] >= 0) & (ix[..., 0] <= 7)
    assert (ix[..., 0][inside] % 1 == 0).any() and (ix[..., 0] % 1 == 0.5).any()
    assert (grid.abs() >= 1e29).any() and not R.any_tap_valid(grid, hi, wi).all()


@pytest.mark.parametrize("name", R.GS_MAPS)
@pytest.mark.parametrize("delta", R.GS_DELTAS)
def test_grid_sample_oracle_passes_its_criterion(name, delta):
    _, _, _, ref32, ref64 = R.gs_case(name, delta)
    assert all(torch.isfinite(t).all() for t in ref32 + ref64)
    R.check_gs(ref32, ref32, ref64)
    close(ref32[0], ref64[0], what="fp32 vs fp64 out")
    close(ref32[1], ref64[1], rel=True, what="fp32 vs fp64 grad_x")
    close(ref32[2], ref64[2], rel=True, what="fp32 vs fp64 grad_grid")


@pytest.mark.parametrize("hw", R.DEGENERATE_INPUTS)
def test_degenerate_inputs(hw):
    x, _, _, grid8, grid9, refs8, refs9 = R.degenerate_case(*hw)
    assert torch.equal(grid9[:, :, :8], grid8[:, :7])
    assert grid8.shape[1] * grid8.shape[2] % 4 == 0 and grid9.shape[1] * grid9.shape[2] % 4 != 0
    # (a one-texel axis keeps a corner inside for |g| < 2: the samples differ in WHICH corner that is)
    x0, y0 = R.corners(grid8, *hw)
    assert R.any_tap_valid(grid8, *hw).any() and x0.unique().numel() >= 2 and y0.unique().numel() >= 2
    if hw[1] == 2:  # the pair origin is pinned to column 0: the corner values are re-assigned on every sample
        assert R.pair_shifts(grid8, *hw).unique().tolist() == [-1, 0, 1]
    for ref32, ref64 in (refs8, refs9):
        R.check_gs(ref32, ref32, ref64)


@pytest.mark.parametrize("shape", R.WIF_SHAPES)
def test_wif_regime_spans_the_gate_and_the_logits(shape):
    b, t, tc, c, co, h, w = shape
    for ab in (True, False):
        vid, net, _, ref32, ref64 = R.wif_case(shape, ab)
        gate = torch.sigmoid(vid[:, :, :, 4] + 5)
        assert gate.min() < 1e-3 and gate.max() > 0.999
        logit = net[:, :, :, 3]
        if tc >= 2:
            finite = torch.isfinite(logit)
            low = torch.where(finite, logit, torch.full_like(logit, float("inf"))).amin(dim=2)
            assert (logit.amax(dim=2) - low).max() > 88 and logit.max() > 89   # exp() alone overflows in fp32
            assert (logit[:, :, 0, R.MASKED_ROW] == float("-inf")).all() and finite[:, :, 1:].all()
            top = logit[:, :, :, R.TIED_ROW].amax(dim=2)
            assert torch.equal(logit[:, :, 0, R.TIED_ROW], top) and torch.equal(logit[:, :, 1, R.TIED_ROW], top)
            assert (ref32[2][:, :, 0, :, R.MASKED_ROW] == 0).all()   # a masked context gets no gradient
        assert all(torch.isfinite(x).all() for x in ref32 + ref64)
        R.check_wif(ref32, ref32, ref64)
        close(ref32[0], ref64[0], what="fp32 vs fp64 out")
        close(ref32[1], ref64[1], rel=True, what="fp32 vs fp64 grad_vid", slice_dims=(3,))
        close(ref32[2], ref64[2], rel=True, what="fp32 vs fp64 grad_net", slice_dims=(3,))


# ------------------------------------------------------------------------------------------ the old operands do not
def _old_occ_operands(nl=32):
    """test_gpu_parity.py:test_occ_composite's."""
    torch.manual_seed(nl)
    m, h, w, div = 6, 9, 31, 3
    alpha = torch.rand(m, nl, h, w)
    occ = torch.rand(m // div, nl, nl)
    return O.occlusion_product(alpha, occ.repeat_interleave(div, dim=0))


def _old_wif_operands(shape=(2, 3, 4, 40, 16, 32, 5)):
    """test_gpu_warper.py:test_wif_fuse_random's (its shapes are (b, t, tc, c, h, w, co))."""
    b, t, tc, c, h, w, co = shape
    torch.manual_seed(c)
    return torch.randn(b, t, tc, c, h, w), torch.randn(b, t, tc, co, h, w)


def test_rand_alphas_hide_the_forward_at_32_layers():
    ref = _old_occ_operands()
    assert (ref < TOL).float().mean() > 0.9
    close(1.01 * ref, ref, what="the whole output times 1.01 under the absolute bound")
    hidden = torch.where(ref < TOL, torch.zeros_like(ref), ref)
    close(hidden, ref, what="outputs below 1e-4 zeroed under the absolute bound")


def test_randn_logits_do_not_need_the_max_subtraction():
    vid, net = _old_wif_operands()
    for ab in (True, False):
        assert (R.wif_fuse_naive(vid, net, ab) - WO.wif_fuse(vid, net, ab)).abs().max() < 1e-6
    gate = torch.sigmoid(_old_wif_operands((1, 2, 5, 8, 33, 65, 4))[0][:, :, :, 4] + 5)
    assert gate.min() > 0.5   # (sigmoid(randn + 5): the gate never closes)


def test_iid_grids_take_neither_wave_uniform_path_nor_make_runs():
    hi, wi = R.GS_INPUT[2:]
    grid = R.iid_map(2, 32, 64, seed=0)
    assert R.spans_all_outside(grid, hi, wi, 256) == 0 and R.spans_all_outside(grid, hi, wi, 64) == 0
    assert R.address_runs(grid, hi, wi).max() <= 3


# ------------------------------------------------------------------------------------------ planted errors
def _rejected(check, got, ref32, ref64):
    with pytest.raises(AssertionError):
        check(got, ref32, ref64)


def test_rejects_small_outputs_of_the_occlusion_product_zeroed():
    _, _, _, ref32, ref64 = R.occ_case(32)
    got = _clone(ref32)
    got[0][got[0] < TOL] = 0
    close(got[0], ref32[0], what="under the absolute bound")   # what test_occ_composite asks
    _rejected(R.check_occ, got, ref32, ref64)


def test_rejects_the_last_layer_of_the_occlusion_product_times_1_01():
    for nl in (21, 32):
        _, _, _, ref32, ref64 = R.occ_case(nl)
        got = _clone(ref32)
        got[0][:, nl - 1] *= 1.01
        _rejected(R.check_occ, got, ref32, ref64)


@pytest.mark.parametrize("shape", [s for s in R.WIF_SHAPES if s[2] >= 2])
def test_rejects_a_softmax_without_max_subtraction(shape):
    vid, net, wgt, ref32, ref64 = R.wif_case(shape, True)
    v, n = vid.clone().requires_grad_(), net.clone().requires_grad_()
    out = R.wif_fuse_naive(v, n, True)
    (out * wgt).sum().backward()
    assert not torch.isfinite(out).all()
    _rejected(R.check_wif, (out.detach(), v.grad, n.grad), ref32, ref64)


def _grid_sample_early_exit_gone_wrong(x, grid, delta):
    """O.grid_sample_delta with ONE planted error: 0 instead of -delta on the 256-pixel pieces without a valid tap."""
    out = O.grid_sample_delta(x, grid, delta)
    mask = R.outside_span_mask(grid, x.shape[2], x.shape[3], 256)
    return out.masked_fill(mask[:, None], 0.0)


@pytest.mark.parametrize("delta", [0.5, 1.0])
def test_rejects_an_early_exit_that_forgets_delta(delta):
    x, grid, _, ref32, ref64 = R.gs_case("affine", delta)
    got = _clone(ref32)
    got[0] = _grid_sample_early_exit_gone_wrong(x, grid, delta)
    assert int((got[0] != ref32[0]).sum()) == 4 * 256 * x.shape[1]
    _rejected(R.check_gs, got, ref32, ref64)
    # on an i.i.d. grid the candidate IS the oracle: no existing single-op test can tell them apart
    iid = R.iid_map(2, 32, 64, seed=0)
    assert torch.equal(_grid_sample_early_exit_gone_wrong(x, iid, delta), O.grid_sample_delta(x, iid, delta))
