"""CPU: the fp64 restatement of the reference scorer's metrics (tests/metrics_ref.py) against scikit-image's numbers
(tests/golden/metrics_skimage.npz, tools_dev/make_metrics_golden.py), waldo_amd.metrics' host side (summarize, argument
checks) and tools.io.load_video_u8."""
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "metrics_skimage.npz")


def test_restatement_matches_skimage():
    g = np.load(GOLDEN)
    assert int(g["n"]) == 3
    for i in range(int(g["n"])):
        a, b = g[f"a{i}"] / 255.0, g[f"b{i}"] / 255.0
        assert abs(R.ssim(a, b) - float(g[f"ssim{i}"])) <= 1e-12, i
        assert abs(R.psnr(a, b) - float(g[f"psnr{i}"])) <= 1e-12, i
    assert max(g["a2"].shape[:2]) >= 161 and g["a2"].shape[0] % 2 == 1


def test_restatement_identities():
    a = np.load(GOLDEN)["a2"] / 255.0
    assert R.msssim(a, a) == pytest.approx(1.0, abs=1e-12)
    assert R.ssim(a, a) == pytest.approx(1.0, abs=1e-12)
    assert R.psnr(a, a) == float("inf")
    for d in (0.5, 0.1, 1 / 255.0):
        assert R.psnr(a, a + d) == pytest.approx(-20 * np.log10(d), abs=1e-9)
    with pytest.raises(ValueError):
        R.msssim(a[:128, :160], a[:128, :160])


def test_downscale_is_symmetric_padding():
    x = np.arange(15.0).reshape(3, 5)
    y = R.downscale(x)
    assert y.shape == (2, 3)
    assert y[1, 2] == x[2, 4]  # the corner: four copies of the last pixel
    assert y[0, 2] == 0.5 * (x[0, 4] + x[1, 4])


def test_summarize_against_hand_table():
    from waldo_amd.metrics import format_lines, summarize
    a = np.array([[1.0, 2.0, 3.0, 4.0],
                  [3.0, 2.0, 5.0, 0.0]])
    s = summarize({"ssim": torch.tensor(a, dtype=torch.float32)}, vid_context=2)
    assert [p["t"] for p in s["ssim"]["per_t"]] == [0, 1, 2, 3]
    assert [(p["mean"], p["std"]) for p in s["ssim"]["per_t"]] == [(2.0, 1.0), (2.0, 0.0), (4.0, 1.0), (2.0, 2.0)]
    # cum at t: clips x frames 2..t -- t = 2: {3, 5}; t = 3: {3, 4, 5, 0}
    assert [c["t"] for c in s["ssim"]["cum"]] == [2, 3]
    assert s["ssim"]["cum"][0]["mean"] == 4.0 and s["ssim"]["cum"][0]["std"] == 1.0
    assert s["ssim"]["cum"][1]["mean"] == 3.0
    assert s["ssim"]["cum"][1]["std"] == pytest.approx(np.sqrt((0 + 1 + 4 + 9) / 4.0), abs=1e-15)
    ref = R.summarize({"ssim": a}, 2)["ssim"]
    assert [(p["mean"], p["std"]) for p in s["ssim"]["per_t"]] == ref["per_t"]
    assert [(c["mean"], c["std"]) for c in s["ssim"]["cum"]] == ref["cum"]
    assert json.loads(json.dumps(s)) == s
    lines = format_lines(s)
    assert lines[0] == "[ssim:0] : (2.0, 1.0)"
    assert "[cum ssim:2] : (4.0, 1.0)" in lines and "[cum ssim:1]" not in " ".join(lines)


def test_frame_metrics_argument_errors_before_the_device():
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    from waldo_amd.metrics import frame_metrics
    x = torch.zeros(1, 2, 3, 64, 64)
    with pytest.raises(ValueError, match="weights"):
        frame_metrics(x, x, metrics=("lpips", "msssim"))
    with pytest.raises(ValueError, match="unknown metric"):
        frame_metrics(x, x, metrics=("fid",))
    small = torch.zeros(1, 2, 3, 128, 256)
    with pytest.raises(ValueError, match="161x161"):
        frame_metrics(small, small)
    with pytest.raises(ValueError, match="8x16"):
        frame_metrics(small, small, metrics=("msssim",))
    with pytest.raises(ValueError, match="differ in shape"):
        frame_metrics(x, torch.zeros(1, 2, 3, 64, 65), metrics=("psnr",))
    with pytest.raises(ValueError, match="channels"):
        frame_metrics(torch.zeros(1, 2, 4, 64, 64), torch.zeros(1, 2, 4, 64, 64), metrics=("psnr",))
    with pytest.raises(ValueError, match="at least 11x11"):
        frame_metrics(torch.zeros(1, 1, 3, 10, 64), torch.zeros(1, 1, 3, 10, 64), metrics=("ssim",))
    with pytest.raises(ValueError, match="quantize"):
        frame_metrics(x, x, metrics=("psnr",), quantize="floor")
    packed = WF.PackedClip(torch.zeros(1, 2, 64, 64, 4, dtype=torch.uint8), 5)
    with pytest.raises(WaldoHipError, match="GPU"):
        frame_metrics(x, packed, metrics=("psnr", "ssim"))
    with pytest.raises(WaldoHipError, match="GPU"):
        frame_metrics(x.to(torch.uint8), x.to(torch.uint8), metrics=("psnr",))


def _clip(seed, t=3, h=20, w=28):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(t, 3, h, w, generator=g) * 2 - 1


@pytest.mark.parametrize("name", ["frames", "clip.png"])
def test_load_video_u8_round_trips_dump_video(tmp_path, name):
    from waldo_amd.tools import io as wio
    v = _clip(1)
    path = str(tmp_path / name)
    wio.dump_video(v, path)
    got = wio.load_video_u8(path)
    assert got.dtype == torch.uint8 and got.shape == (3, 3, 20, 28)
    want = ((v - -1.0) / 2.0).clamp(0, 1).mul(255.0).add(0.5).to(torch.uint8)
    assert torch.equal(got, want)


def test_load_video_u8_refuses_mp4_and_empty(tmp_path):
    from waldo_amd.tools import io as wio
    with pytest.raises(ValueError, match="mp4"):
        wio.load_video_u8(str(tmp_path / "x.mp4"))
    with pytest.raises(ValueError, match="no PNG"):
        wio.load_video_u8(str(tmp_path))


def test_entry_point_checks_arguments_without_a_gpu():
    """The C ABI's workspace sizes and its refusals come from the host, before any launch."""
    from waldo_amd import _lib
    lib = _lib.load()
    # scale 0 only: one (lum*cs, cs, squared error) triple per 32 x 64 tile of each (frame, channel)
    assert lib.waldo_frame_metrics_partial_bytes(2, 3, 64, 128, 3) == 2 * 3 * 3 * (2 * 2) * 3 * 8
    assert lib.waldo_frame_metrics_scratch_bytes(2, 3, 64, 128, 3) == 0
    # MS-SSIM: four more scales, each a pooled copy of both operands
    sides = [(181, 243), (91, 122), (46, 61), (23, 31), (12, 16)]
    pooled = sum(2 * 6 * 3 * h * w for h, w in sides[1:])
    assert lib.waldo_frame_metrics_scratch_bytes(2, 3, 181, 243, 7) == pooled * 4
    assert lib.waldo_frame_metrics_partial_bytes(2, 3, 64, 128, 0) == -1
    args = [None, 0, 0, 0, 0, 0, None, 0, 0, 0, 0, 0, None]
    assert lib.waldo_frame_metrics_fwd(*args, 1, 1, 128, 256, -1.0, 2.0, 0, 7, *([None] * 5), None) == -1
    assert b"161" in lib.waldo_last_error_string()
    assert lib.waldo_frame_metrics_fwd(*args, 1, 1, 10, 64, -1.0, 2.0, 0, 2, *([None] * 5), None) == -1
    assert lib.waldo_frame_metrics_fwd(*args[:1], 5, *args[2:], 1, 1, 64, 64, -1.0, 2.0, 0, 1, *([None] * 5),
                                       None) == -1
    assert b"encoding" in lib.waldo_last_error_string()
    assert lib.waldo_frame_metrics_fwd(*args, 1, 1, 64, 64, -1.0, 0.0, 0, 1, *([None] * 5), None) == -1
    assert lib.waldo_frame_metrics_fwd(*args, 1, 1, 64, 64, -1.0, 2.0, 0, 1, *([None] * 5), None) == -1
    assert b"null" in lib.waldo_last_error_string()
    assert lib.waldo_frame_metrics_fwd(*args, 0, 4, 64, 64, -1.0, 2.0, 0, 1, *([None] * 5), None) == 0
