"""CPU: what tests/test_gpu_metrics_regimes.py rests on, shown from the restatements alone (tests/metrics_regimes.py
against tests/metrics_ref.py): the new operands reach the ill-conditioned regime and the old ones do not; fp32 in
TF's operation order misses the project's bound there and the shifted form the pass kernel uses keeps it; the signs
the MS-SSIM relu meets are there; and the criterion rejects planted faults at the operands and shapes the GPU file
uses."""
import numpy as np
import pytest

import metrics_ref as R
import metrics_regimes as M

H, W = M.SSIM_HW


def _pair(a, d, f=0):
    return M.unit(d)[0, f], M.unit(a)[0, f]


def test_regimes_hold():
    for name in M.BRIGHT:
        assert M.median_kappa(*M.regime(name, 1, 2, H, W)) >= 1000, name
    # the operands of tests/test_gpu_metrics.py do not reach the regime, at any of its shapes
    for h, w, seed in ((75, 139, 1), (181, 243, 1), (37, 53, 4)):
        assert M.median_kappa(*M.textured(1, 2, h, w, seed)) < 100, (h, w)
    assert M.median_kappa(*M.regime("dark_flat", 1, 2, H, W)) < 10
    # mixed_tile: a bright, flat half and a textured half in every tile
    a, d = M.regime("mixed_tile", 1, 2, H, W)
    k = M.kappa(M.unit(a)[0, 0, 0], M.unit(d)[0, 0, 0])
    assert np.median(k[:, :16]) >= 1000 and np.median(k[:, 36:48]) < 100
    assert int((a[..., 32:64].int() - d[..., 32:64].int()).abs().max()) <= 6


def test_tf_order_in_fp32_is_fine_on_textured_frames():
    for h, w in ((75, 139), (181, 243)):
        p, r = _pair(*M.textured(1, 1, h, w, seed=1))
        ref = R.ssim(p, r, chw=True)
        assert abs(M.tf_order_fp32(p, r) - ref) <= 0.01 * M.TOL_SSIM  # 1e-8 ... 4e-8
        assert abs(M.shifted_fp32(p, r) - ref) <= 0.01 * M.TOL_SSIM


@pytest.mark.parametrize("name", ["bright255_sd1", "bright250_sd1", "bright235_sd1"])
def test_tf_order_in_fp32_misses_the_bound_on_bright_flat_frames(name):
    """2.7e-5 ... 4.2e-5 off fp64, the same sign in every frame: at least twice the bound.  The shifted form stays
    1000 times closer."""
    a, d = M.regime(name, 1, 2, H, W)
    errs = []
    for f in range(2):
        p, r = _pair(a, d, f)
        ref = R.ssim(p, r, chw=True)
        errs.append(M.tf_order_fp32(p, r) - ref)
        assert abs(errs[-1]) >= 2 * M.TOL_SSIM, (name, errs)
        assert abs(M.shifted_fp32(p, r) - ref) <= 0.01 * M.TOL_SSIM, name
    assert errs[0] * errs[1] > 0  # systematic


def test_shifted_form_keeps_the_bound_on_every_regime():
    worst = {}
    for name in M.REGIMES:
        a, d = M.regime(name, 1, 2, H, W)
        p, r = M.unit(d), M.unit(a)
        worst[name] = M.fractions(M.restated(p, r, ("psnr", "ssim")), M.reference(p, r, ("psnr", "ssim")))
    print(worst)
    assert all(v <= 1.0 for fr in worst.values() for v in fr.values()), worst
    # no single constant per tile is near both halves of mixed_tile, yet a tenth of the bound is kept
    assert worst["mixed_tile"]["ssim"] <= 0.2, worst["mixed_tile"]


def test_shifted_form_msssim():
    for name in ("bright235_sd1", "mixed_tile"):
        a, d = M.regime(name, 1, 2, *M.MS_HW)
        p, r = M.unit(d)[:, :1], M.unit(a)[:, :1]
        ref = M.reference(p, r, ("msssim",))
        assert M.fractions(M.restated(p, r, ("msssim",)), ref)["msssim"] <= 0.1, name
        if name == "bright235_sd1":  # TF's order: -3.7e-5 before the powers, still past the bound after them
            assert M.fractions(M.restated(p, r, ("msssim",), shift=False), ref)["msssim"] >= 2.0


def test_equal_frames_score_exactly_one():
    for name in ("bright255_sd1", "mixed_tile", "inverted"):
        p = M.unit(M.regime(name, 1, 2, H, W)[0])[0, 0]
        assert M.shifted_fp32(p, p) == 1.0 and M.tf_order_fp32(p, p) == 1.0, name
        assert M.psnr_fp32(p, p) == float("inf")
    p, r = _pair(*M.regime("bright235_sd1", 1, 2, H, W))
    assert M.shifted_fp32(p, r) == M.shifted_fp32(r, p)  # commutative


def test_inverted_frames():
    a, d = M.regime("inverted", 1, 2, *M.MS_HW)
    p, r = _pair(a, d)
    assert R.msssim(p, r, chw=True) == 0.0 and M.shifted_fp32_ms(p, r) == 0.0 and M.tf_order_fp32_ms(p, r) == 0.0
    assert R.ssim(p, r, chw=True) < -0.9 and M.shifted_fp32(p, r) < -0.9
    for c in range(3):  # the mean cs is negative while the pooled noise is large against C2: one zero factor is enough
        x, y = p[c].astype(np.float64), r[c].astype(np.float64)
        for k in range(3):
            assert R.ssim_channel(x, y)[1] < -0.5, (c, k)
            x, y = R.downscale(x), R.downscale(y)


@pytest.mark.parametrize("hw", [M.SSIM_HW, M.MS_HW])
def test_near_zero_cs_has_the_three_signs(hw):
    a, d = M.regime("near_zero_cs", 1, 2, *hw)
    for f in range(2):
        p, r = _pair(a, d, f)
        cs = [R.ssim_channel(p[c].astype(np.float64), r[c].astype(np.float64))[1] for c in range(3)]
        assert cs[0] < -0.05 and cs[1] > 0.05 and abs(cs[2]) < 1e-3, cs


def test_single_pixel():
    a, d, (c, y, x) = M.single_pixel(2, 3, 64, 128, seed=22, frame=(1, 1))
    diff = (a.int() - d.int()).abs()
    assert int(diff.sum()) == 1 and int(diff[1, 1, c, y, x]) == 1


def test_fp32_rendition_is_not_byte_quantised():
    a, _ = M.regime("bright250_sd1", 1, 2, H, W)
    u = R.quantize(M.as_fp32(a, 1).numpy(), M.SPAN, "none") * 255.0
    off = u - a.numpy()
    assert np.abs(off).max() <= 0.401 and off.std() > 0.2
    assert np.mean(np.abs(u - np.rint(u)) > 0.05) > 0.8


# ------------------------------------------------------------------------------------------------------ planted faults
def _rejected(p, r, metrics, fault):
    """The GPU file's criterion passes the restatement and fails it with ``fault`` planted, on the same operands."""
    ref = M.reference(p, r, metrics)
    clean = M.fractions(M.restated(p, r, metrics), ref)
    bad = M.fractions(M.restated(p, r, metrics, fault=fault), ref)
    assert all(v <= 1.0 for v in clean.values()), (fault, clean)
    return any(not v <= 1.0 for v in bad.values())


@pytest.mark.parametrize("hw", [(11, 11), (42, 74), (43, 75), (32, 64), (64, 128)])
def test_criterion_rejects_a_valid_map_one_row_too_long(hw):
    a, d = M.textured(1, 1, *hw, seed=20)
    assert _rejected(M.unit(d), M.unit(a), ("ssim",), "valid_row"), hw


def test_criterion_rejects_zero_padding_at_an_odd_side():
    a, d = M.textured(1, 1, 161, 161, seed=23)
    assert _rejected(M.unit(d), M.unit(a), ("msssim",), "zero_pad")
    a, d = M.regime("bright235_sd1", 1, 2, *M.MS_HW)
    assert _rejected(M.unit(d)[:, :1], M.unit(a)[:, :1], ("msssim",), "zero_pad")


@pytest.mark.parametrize("name", ["inverted", "near_zero_cs"])
def test_criterion_rejects_a_missing_relu(name):
    a, d = M.regime(name, 1, 2, *M.MS_HW)
    assert _rejected(M.unit(d)[:, :1], M.unit(a)[:, :1], ("msssim",), "no_relu")


@pytest.mark.parametrize("name", ["bright250_sd1", "flat240_vs_sd3", "dark_flat", "mixed_tile"])
def test_criterion_rejects_c2_off_by_one_percent(name):
    a, d = M.regime(name, 1, 2, H, W)
    assert _rejected(M.unit(d)[:, :1], M.unit(a)[:, :1], ("ssim",), "c2")


def test_criterion_rejects_a_wrong_centre_tap():
    """The unnormalised centre tap off by 1e-3 changes every weight by 3e-4 of itself at the most.  Over a map of many
    windows that averages out (0.02 ... 0.5 of the bound on the regimes at 75 x 139): the frame with ONE output shows it."""
    a, d = M.textured(1, 2, 11, 11, seed=20)
    assert _rejected(M.unit(d), M.unit(a), ("ssim",), "centre_tap")


@pytest.mark.parametrize("hw", [(3, 5), (10, 200), (33, 65), (64, 128)])
def test_criterion_rejects_a_squared_error_summed_over_the_apron(hw):
    a, d = M.textured(1, 1, *hw, seed=21)
    rejected = _rejected(M.unit(d), M.unit(a), ("psnr",), "apron_se")
    # a frame inside one tile has no pixel in another tile's apron: only frames of more than one tile can show it
    assert rejected == (hw[0] > M.TILE_H or hw[1] > M.TILE_W), hw
