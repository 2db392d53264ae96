"""GPU: waldo_amd.metrics.frame_metrics on the operands of tests/metrics_regimes.py -- bright and flat windows, where
SSIM's variance term cancels, negative and near-zero cs -- and at the shapes where the VALID map, the 32 x 64 tile and
the 2 x 2 pooling meet.  Every comparison is against the fp64 restatement (tests/metrics_ref.py), per frame, at the
project's TOL_SSIM / TOL_PSNR; the bit-exact identities of tests/test_gpu_metrics.py are asserted on the new operands.
Run with ``-s`` for the worst |kernel - fp64| of every regime as a fraction of its bound."""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
import metrics_regimes as M

pytestmark = pytest.mark.gpu

ENCODINGS = ("u8", "packed", "f32")
ALL = ("psnr", "ssim", "msssim")
_WORST = {}  # regime -> metric -> the worst fraction of the bound seen, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |kernel - fp64| as a fraction of the bound (TOL_SSIM 1e-5, TOL_PSNR 1e-4):")
    for name, fr in _WORST.items():
        print(f"  {name:32s} " + "  ".join(f"{m} {v:.3f}" for m, v in fr.items()))


def _encode(u8, enc, dev, seed):
    """(operand on the device, quantize mode, the [0, 1] fp32 clip the kernel scores for it)."""
    from waldo_amd import functional as WF
    if enc == "u8":
        return u8.to(dev), "round", M.unit(u8)
    if enc == "packed":  # a packed clip under "round" gives back its bytes
        cls = torch.zeros(u8.shape[:2] + u8.shape[3:], dtype=torch.uint8)
        return WF.pack_clip(u8.to(dev), cls.to(dev), 3), "round", M.unit(u8)
    x = M.as_fp32(u8, seed)
    return x.to(dev), "none", R.quantize(x.numpy(), M.SPAN, "none")


@functools.lru_cache(maxsize=None)
def _reference(name, enc, hw, metrics):
    """The fp64 scores of a regime's operands, computed once: "u8" and "packed" score the same bytes."""
    a, d = M.regime(name, 1, 2, *hw)
    if enc == "f32":
        p, r = (R.quantize(M.as_fp32(x, s).numpy(), M.SPAN, "none") for x, s in ((d, 1), (a, 2)))
    else:
        p, r = M.unit(d), M.unit(a)
    return M.reference(p, r, metrics)


def _scores(pred, real, quant, metrics):
    from waldo_amd.metrics import frame_metrics
    got = frame_metrics(pred, real, metrics=metrics, quantize=quant)
    torch.cuda.synchronize()
    for v in got.values():
        assert v.dtype == torch.float32 and v.shape == tuple(pred.shape[:2])
    return {m: v.cpu().numpy() for m, v in got.items()}


def _judge(label, got, ref):
    fr = M.fractions(got, ref)
    print(label, {m: round(v, 4) for m, v in fr.items()})
    seen = _WORST.setdefault(label.split("[")[0], {})
    for m, v in fr.items():
        seen[m] = max(seen.get(m, 0.0), v)
    assert all(v <= 1.0 for v in fr.values()), (label, fr)
    return fr


def _check(label, pred_u8, real_u8, encs, dev, metrics):
    pred, q, p = _encode(pred_u8, encs[0], dev, 1)
    real, q2, r = _encode(real_u8, encs[1], dev, 2)
    quant = "none" if "none" in (q, q2) else "round"
    return _judge(label, _scores(pred, real, quant, metrics), M.reference(p, r, metrics))


# ------------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("enc", ENCODINGS)
@pytest.mark.parametrize("name", list(M.REGIMES))
def test_conditioning_ssim(dev, name, enc):
    a, d = M.regime(name, 1, 2, *M.SSIM_HW)
    metrics = ("psnr", "ssim")
    pred, quant, _ = _encode(d, enc, dev, 1)
    real, _, _ = _encode(a, enc, dev, 2)
    _judge(f"{name}[{enc} 75x139]", _scores(pred, real, quant, metrics), _reference(name, enc, M.SSIM_HW, metrics))


@pytest.mark.parametrize("enc", ENCODINGS)
@pytest.mark.parametrize("name", list(M.REGIMES))
def test_conditioning_msssim(dev, name, enc):
    a, d = M.regime(name, 1, 2, *M.MS_HW)
    pred, quant, _ = _encode(d, enc, dev, 1)
    real, _, _ = _encode(a, enc, dev, 2)
    _judge(f"{name}[{enc} 161x193]", _scores(pred, real, quant, ALL), _reference(name, enc, M.MS_HW, ALL))


# ---------------------------------------------------------------------------------------------------------- geometry
# 11 x 11: one output.  42 x 74: Wv = 64 and Hv = 32, the second tile row and column own pixels but no output; 43 x 75:
# one output row and column in them.  64 x 128: exact tiles, the last tile's apron wholly outside the frame.
@pytest.mark.parametrize("hw", [(11, 11), (11, 75), (43, 11), (42, 74), (43, 75), (33, 65), (32, 64), (64, 128)])
@pytest.mark.parametrize("encs", [("f32", "u8"), ("packed", "f32")])
def test_geometry(dev, hw, encs):
    a, d = M.textured(1, 2, *hw, seed=20)
    _check(f"geometry {hw[0]}x{hw[1]}[{encs[0]} {encs[1]}]", d, a, encs, dev, ("psnr", "ssim"))


# -------------------------------------------------------------------------------------------------------------- PSNR
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (10, 200)])
@pytest.mark.parametrize("encs", [("f32", "u8"), ("u8", "packed")])
def test_psnr_below_the_window(dev, hw, encs):
    a, d = M.textured(2, 3, *hw, seed=21)
    _check(f"psnr {hw[0]}x{hw[1]}[{encs[0]} {encs[1]}]", d, a, encs, dev, ("psnr",))


def test_psnr_black_against_white_is_0_db(dev):
    z = torch.zeros(1, 2, 3, 33, 65, dtype=torch.uint8)
    got = _scores(z.to(dev), (z + 255).to(dev), "trunc", ("psnr",))["psnr"]
    assert np.all(np.abs(got) <= M.TOL_PSNR), got


@pytest.mark.parametrize("enc", ["u8", "packed"])
def test_psnr_single_pixel(dev, enc):
    h, w = 64, 128
    a, d, _ = M.single_pixel(2, 3, h, w, seed=22, frame=(1, 1))
    pred, quant, _ = _encode(d, enc, dev, 1)
    real, _, _ = _encode(a, enc, dev, 2)
    got = _scores(pred, real, quant, ("psnr", "ssim"))
    want = -10.0 * math.log10((1.0 / 255.0) ** 2 / (3 * h * w))
    assert abs(got["psnr"][1, 1] - want) <= M.TOL_PSNR, (got["psnr"][1, 1], want)
    others = np.ones((2, 3), bool)
    others[1, 1] = False
    assert np.all(got["psnr"][others] == np.inf), got["psnr"]  # the neighbouring frames of the same call
    assert np.all(got["ssim"][others] == 1.0), got["ssim"]
    _judge(f"single_pixel 64x128[{enc}]", got, M.reference(M.unit(d), M.unit(a), ("psnr", "ssim")))


# ----------------------------------------------------------------------------------------------------------- MS-SSIM
@pytest.mark.parametrize("hw", [(161, 161), (162, 176)])
@pytest.mark.parametrize("encs", [("f32", "packed"), ("u8", "f32")])
def test_msssim_sizes(dev, hw, encs):
    a, d = M.textured(1, 2, *hw, seed=23)
    _check(f"msssim {hw[0]}x{hw[1]}[{encs[0]} {encs[1]}]", d, a, encs, dev, ALL)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_msssim_of_inverted_frames_is_exactly_zero(dev, enc):
    a, d = M.regime("inverted", 1, 2, *M.MS_HW)
    pred, quant, _ = _encode(d, enc, dev, 1)
    real, _, _ = _encode(a, enc, dev, 2)
    got = _scores(pred, real, quant, ("ssim", "msssim"))
    assert np.all(got["msssim"] == 0.0), got["msssim"]
    assert np.all(got["ssim"] < -0.9), got["ssim"]


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_msssim_near_zero_cs_per_channel(dev, channel):
    """The three channels of the clip hold one channel of ``near_zero_cs``, so the score is that channel's: its mean cs
    at scale 0 is negative (MS-SSIM 0), positive, or within 1e-3 of zero (the relu decides on the sign of a sum that
    nearly cancels)."""
    a, d = (x[:, :, channel:channel + 1].expand(-1, -1, 3, -1, -1).contiguous()
            for x in M.regime("near_zero_cs", 1, 2, *M.MS_HW))
    p, r = M.unit(d), M.unit(a)
    for f in range(2):
        cs0 = R.ssim_channel(p[0, f, 0].astype(np.float64), r[0, f, 0].astype(np.float64))[1]
        assert (cs0 < -0.05, cs0 > 0.05, abs(cs0) < 1e-3)[channel], (channel, cs0)
    _judge(f"near_zero_cs channel {channel}[u8 161x193]", _scores(d.to(dev), a.to(dev), "round", ALL),
           M.reference(p, r, ALL))


MIXED_CALL = ("bright255_sd1", "dark_flat", "inverted", "equal", "mixed_tile", "near_zero_cs")


@pytest.mark.parametrize("enc", ENCODINGS)
def test_one_call_with_every_regime(dev, enc):
    """A (2, 3) clip whose frames are of different regimes (one of them with equal frames): a slip in a frame or channel
    index gives some frame another frame's score, far from its own."""
    pairs = [M.regime("bright255_sd1" if n == "equal" else n, 1, 2, *M.MS_HW) for n in MIXED_CALL]
    a = torch.stack([x[0][0, k % 2] for k, x in enumerate(pairs)]).view(2, 3, 3, *M.MS_HW)
    d = torch.stack([x[1][0, k % 2] for k, x in enumerate(pairs)]).view(2, 3, 3, *M.MS_HW).clone()
    d[1, 0] = a[1, 0]  # "equal"
    pred, quant, p = _encode(d, enc, dev, 1)
    real, _, r = _encode(a, enc, dev, 1)  # the same jitter: the equal frames stay equal in fp32
    got = _scores(pred, real, quant, ALL)
    ref = M.reference(p, r, ALL)
    assert len({round(float(v), 3) for v in ref["ssim"].ravel()}) == 6  # no two frames score alike
    assert got["psnr"][1, 0] == np.inf and got["ssim"][1, 0] == 1.0 and got["msssim"][1, 0] == 1.0
    assert got["msssim"][0, 2] == 0.0  # inverted
    _judge(f"one call, six regimes[{enc} 161x193]", got, ref)


# -------------------------------------------------------------------------------------------------- kept identities
@pytest.mark.parametrize("hw", [M.SSIM_HW, M.MS_HW])
@pytest.mark.parametrize("name", list(M.REGIMES))
def test_bit_identities(dev, name, hw):
    from waldo_amd.metrics import frame_metrics
    metrics = ALL if hw == M.MS_HW else ("psnr", "ssim")
    a, d = M.regime(name, 1, 2, *hw)
    bits = lambda x: {m: v.cpu().numpy().view(np.uint32) for m, v in x.items()}  # noqa: E731
    same = lambda x, y: all(np.array_equal(x[m], y[m]) for m in x)  # noqa: E731
    for enc in ENCODINGS:
        pred, quant, _ = _encode(d, enc, dev, 1)
        real, _, _ = _encode(a, enc, dev, 2)
        x = bits(frame_metrics(pred, real, metrics=metrics, quantize=quant))
        assert same(x, bits(frame_metrics(pred, real, metrics=metrics, quantize=quant))), (enc, "two calls")
        assert same(x, bits(frame_metrics(real, pred, metrics=metrics, quantize=quant))), (enc, "(a, b) and (b, a)")
        if enc == "u8":
            u8_bits = x
        if enc == "packed":
            assert same(x, u8_bits), "u8 and packed under round"
        # equal frames: exactly 1.0 and +inf
        e = frame_metrics(real, real, metrics=metrics, quantize=quant)
        assert bool((e["psnr"] == float("inf")).all()), (enc, e["psnr"])
        assert bool((e["ssim"] == 1.0).all()), (enc, e["ssim"])
        if "msssim" in e:
            assert bool((e["msssim"] == 1.0).all()), (enc, e["msssim"])
