"""GPU: waldo_amd.metrics.frame_metrics (csrc/frame_metrics.hip) against the fp64 restatement of the reference scorer's
metrics (tests/metrics_ref.py), its bit-exact identities, tools.evaluate as a child process and demo --eval."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = os.path.join(ROOT, "tests", "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")
SPAN = (-1.0, 1.0)
TOL_SSIM, TOL_PSNR = 1e-5, 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bytes(b, t, h, w, seed):
    """A smooth clip with texture (uint8, (B, T, 3, H, W)) and a distorted copy of it."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b * t, 3, h // 8 + 2, w // 8 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(coarse, scale_factor=8, mode="bilinear")[..., :h, :w]
    a = (0.7 * smooth + 0.3 * torch.rand(b * t, 3, h, w, generator=g)).clamp(0, 1)
    d = (a + 0.05 * torch.randn(a.shape, generator=g) + 0.02).clamp(0, 1)
    cvt = lambda x: (x * 255 + 0.5).to(torch.uint8).view(b, t, 3, h, w)  # noqa: E731
    return cvt(a), cvt(d)


def _operand(u8, enc, dev, seed=0):
    """The clip of bytes ``u8`` as an fp32 clip (values that quantise near those bytes, a few outside the span), a uint8
    clip or a PackedClip."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.io import rgb_from_u8
    if enc == "u8":
        return u8.to(dev)
    if enc == "packed":
        cls = torch.zeros(u8.shape[:2] + u8.shape[3:], dtype=torch.uint8)
        return WF.pack_clip(u8.to(dev), cls.to(dev), 3)
    g = torch.Generator().manual_seed(seed)
    x = rgb_from_u8(u8) + 0.004 * torch.randn(u8.shape, generator=g)
    x.view(-1)[:: 997] = 1.25
    return x.to(dev)


def _unit(op, quant):
    """The fp32 [0, 1] frames ``frame_metrics`` scores, (B, T, 3, H, W) numpy."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.io import rgb_from_u8
    if isinstance(op, WF.PackedClip):
        return R.quantize(rgb_from_u8(op.data[..., :3].permute(0, 1, 4, 2, 3).cpu()).numpy(), SPAN, quant)
    if op.dtype == torch.uint8:
        return op.cpu().numpy().astype(np.float32) / np.float32(255)
    return R.quantize(op.cpu().numpy(), SPAN, quant)


def _check(pred, real, quant, metrics=("psnr", "ssim", "msssim")):
    from waldo_amd.metrics import frame_metrics
    got = frame_metrics(pred, real, metrics=metrics, quantize=quant)
    torch.cuda.synchronize()
    p, r = _unit(pred, quant), _unit(real, quant)
    b, t = p.shape[:2]
    for i in range(b):
        for j in range(t):
            fp, fr = p[i, j], r[i, j]
            if "psnr" in metrics:
                assert abs(got["psnr"][i, j].item() - R.psnr(fp, fr)) <= TOL_PSNR, (i, j)
            if "ssim" in metrics:
                assert abs(got["ssim"][i, j].item() - R.ssim(fp, fr, chw=True)) <= TOL_SSIM, (i, j)
            if "msssim" in metrics:
                assert abs(got["msssim"][i, j].item() - R.msssim(fp, fr, chw=True)) <= TOL_SSIM, (i, j)
    for v in got.values():
        assert v.shape == (b, t) and v.dtype == torch.float32 and not v.requires_grad
    return got


@pytest.mark.parametrize("quant", ["trunc", "round", "none"])
@pytest.mark.parametrize("encs", [("f32", "packed"), ("packed", "u8"), ("u8", "f32")])
def test_encodings_and_quantisations(dev, encs, quant):
    a, b = _bytes(1, 2, 181, 243, seed=1)
    _check(_operand(b, encs[0], dev, seed=2), _operand(a, encs[1], dev, seed=3), quant)


@pytest.mark.parametrize("shape", [(1, 2, 37, 53), (1, 1, 256, 832), (1, 2, 512, 1024)])
def test_sizes(dev, shape):
    a, b = _bytes(*shape, seed=4)
    metrics = ("psnr", "ssim") if shape[2] < 161 else ("psnr", "ssim", "msssim")
    _check(_operand(b, "f32", dev, seed=5), _operand(a, "packed", dev), "trunc", metrics)


def test_strided_fp32_view(dev):
    a, b = _bytes(2, 2, 181, 243, seed=6)
    wide = torch.randn(2, 2, 23, 181, 243, device=dev)
    wide[:, :, :3] = _operand(b, "f32", dev, seed=7)
    view = wide[:, :, :3]
    assert not view.is_contiguous()
    _check(view, _operand(a, "u8", dev), "round")


def test_bit_identities(dev):
    from waldo_amd.metrics import frame_metrics
    a, b = _bytes(2, 2, 181, 243, seed=8)
    packed = _operand(a, "packed", dev)
    pred = _operand(b, "f32", dev, seed=9)
    for quant in ("trunc", "round", "none"):
        x = frame_metrics(pred, packed, quantize=quant)
        y = frame_metrics(pred, packed.unpack()[:, :, :3], quantize=quant)
        for k in x:
            assert torch.equal(x[k], y[k]), (quant, k)
    # a packed clip under "round" gives back its bytes: the same bits as the uint8 clip of them
    x = frame_metrics(pred, packed, quantize="round")
    y = frame_metrics(pred, a.to(dev), quantize="round")
    z = frame_metrics(pred, packed, quantize="round")
    w = frame_metrics(packed, pred, quantize="round")
    for k in x:
        assert torch.equal(x[k], y[k]) and torch.equal(x[k], z[k]) and torch.equal(x[k], w[k]), k
    # the default quantisation differs: the reference's dump_video truncates
    assert not torch.equal(frame_metrics(pred, packed)["psnr"], x["psnr"])


def test_round_equals_dumped_png_frames(dev, tmp_path):
    from waldo_amd.metrics import frame_metrics
    from waldo_amd.tools import io as wio
    a, b = _bytes(1, 3, 181, 243, seed=10)
    pred, real = _operand(b, "f32", dev, seed=11), _operand(a, "f32", dev, seed=12)
    x = frame_metrics(pred, real, quantize="round")
    wio.dump_video(pred[0], str(tmp_path / "pred"))
    wio.dump_video(real[0], str(tmp_path / "real"))
    pu = wio.load_video_u8(str(tmp_path / "pred"))[None].to(dev)
    ru = wio.load_video_u8(str(tmp_path / "real"))[None].to(dev)
    y = frame_metrics(pu, ru)
    for k in x:
        assert torch.equal(x[k], y[k]), k


def test_equal_frames(dev):
    from waldo_amd.metrics import frame_metrics
    a, _ = _bytes(1, 1, 161, 161, seed=13)
    x = frame_metrics(a.to(dev), a.to(dev))
    assert x["psnr"].item() == float("inf")
    assert x["ssim"].item() == pytest.approx(1.0, abs=1e-6)
    assert x["msssim"].item() == pytest.approx(1.0, abs=1e-6)


def test_evaluate_cli_json(dev, tmp_path):
    from waldo_amd.metrics import frame_metrics, summarize
    from waldo_amd.tools import io as wio
    a, b = _bytes(3, 4, 48, 64, seed=14)
    for name, clips in (("real", a), ("fake", b)):
        for i in range(clips.shape[0]):
            wio.dump_video(wio.rgb_from_u8(clips[i]), str(tmp_path / name / f"clip{i:02d}"))
    out = tmp_path / "scores.json"
    r = subprocess.run([sys.executable, "-m", "waldo_amd.tools.evaluate", str(tmp_path / "real"), str(tmp_path / "fake"),
                        "4", "2", "--metrics", "psnr", "ssim", "--batch-size", "2", "--json", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[ssim:3] : (" in r.stdout and "[cum psnr:3] : (" in r.stdout and "note: scoring all 3" in r.stdout
    want = summarize(frame_metrics(b.to(dev), a.to(dev), metrics=("psnr", "ssim")), 2)
    assert json.loads(out.read_text()) == want


def test_demo_eval_packed_and_fp32(dev):
    from waldo_amd.tools import demo
    ctx_len = 4  # demo.run's default
    got = [demo.run(CLIP, dim=128, device=str(dev), packed=p, eval=True, ctx_len=ctx_len)["metrics"]
           for p in (False, True)]
    assert set(got[0]) == {"rec_vid", "inp_pred_vid"}
    for key in got[0]:
        assert set(got[0][key]) == {"psnr", "ssim"}  # MS-SSIM: not applicable at 128 x 128
        for m, v in got[0][key].items():
            assert torch.equal(v, got[1][key][m]), (key, m)
            # inp_pred_vid's context frames ARE the real frames: PSNR +inf there (TF's value), finite elsewhere
            finite = v[:, ctx_len:] if (key, m) == ("inp_pred_vid", "psnr") else v
            assert bool(torch.isfinite(finite).all()), (key, m)
        s = got[0][key]["ssim"]
        assert bool(((s > -1) & (s <= 1)).all())
    assert bool((got[0]["inp_pred_vid"]["psnr"][:, :ctx_len] == float("inf")).all())
    assert bool((got[0]["inp_pred_vid"]["ssim"][:, :ctx_len] == 1.0).all())
