"""CPU: the C ABI and the Python surface of the byte output (include/waldo_hip.h "Byte output":
waldo_frames_to_bytes_fwd, waldo_wif_fuse_bytes_fwd / _dt; functional.frames_to_bytes / wif_fuse_bytes; out_bytes of
WIF and tools.demo; tools.io's writers).  No kernel is launched and no GPU is touched: every check here is argument
validation on the host, or host-side file writing."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32, F16, BF16, PACKED = 0, 1, 2, 3
NCHW, NHWC = 0, 1
TRUNC, ROUND, NONE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def f2b(lib, src=1, code=F32, ss=(48, 16, 4), table=None, dst=1, ds_n=48, layout=NCHW, n=1, c=3, h=4, w=4, lo=-1.0,
        rng=2.0, quant=TRUNC):
    """waldo_frames_to_bytes_fwd with one argument off; the pointers are never dereferenced (every case is refused, or
    returns, before a launch)."""
    return lib.waldo_frames_to_bytes_fwd(src, code, *ss, table, dst, ds_n, layout, n, c, h, w, lo, rng, quant, None)


def test_version_is_unchanged(lib):
    assert lib.waldo_version() == 1020


@pytest.mark.parametrize("kw,msg", [
    (dict(code=4), b"unknown dtype"), (dict(code=-1), b"unknown dtype"),
    (dict(layout=2), b"unknown layout"), (dict(layout=-1), b"unknown layout"),
    (dict(quant=NONE), b"unknown quantisation"), (dict(quant=-1), b"unknown quantisation"),
    (dict(rng=0.0), b"bad span"), (dict(rng=-2.0), b"bad span"), (dict(rng=float("inf")), b"bad span"),
    (dict(rng=float("nan")), b"bad span"), (dict(lo=float("nan")), b"bad span"), (dict(lo=float("-inf")), b"bad span"),
    (dict(ss=(-48, 16, 4)), b"negative stride"), (dict(ss=(48, -16, 4)), b"negative stride"),
    (dict(ss=(48, 16, -4)), b"negative stride"), (dict(ds_n=-48), b"negative stride"),
    (dict(layout=NHWC, c=4), b"3 channels"), (dict(layout=NHWC, c=1), b"3 channels"),
    (dict(code=PACKED, c=4, table=1), b"3 channels"),
    (dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"),
    (dict(code=PACKED, table=None, src=4), b"null pointer"),
    (dict(src=2), b"not aligned"), (dict(code=F16, src=1), b"not aligned"), (dict(code=PACKED, table=1, src=2), b"not aligned"),
    (dict(n=-1), b"bad shape"), (dict(c=0), b"bad shape"), (dict(h=0), b"bad shape"), (dict(w=0), b"bad shape"),
    (dict(w=32769), b"bad shape"),
    (dict(n=2 ** 31, src=4), b"too large"),            # one workgroup per frame: a grid of 2^31
    (dict(n=2 ** 40, h=32768, w=32768, src=4), b"too large"),
])
def test_frames_to_bytes_rejects_bad_arguments(lib, kw, msg):
    kw.setdefault("src", 4)
    assert f2b(lib, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


def test_empty_batch_returns_ok_without_a_launch(lib):
    assert f2b(lib, n=0, src=None, dst=None) == 0
    assert f2b(lib, n=0, src=None, dst=None, code=PACKED, layout=NHWC) == 0
    assert lib.waldo_wif_fuse_bytes_fwd(None, None, None, 0, 4, 5, 4, 64, 1, -1.0, 2.0, TRUNC, NCHW, None) == 0
    assert lib.waldo_wif_fuse_bytes_fwd_dt(None, None, None, 0, 4, 5, 4, 64, 1, -1.0, 2.0, ROUND, NHWC, BF16, F16,
                                           None) == 0


def test_wif_fuse_bytes_rejects_bad_arguments(lib):
    fwd, dt = lib.waldo_wif_fuse_bytes_fwd, lib.waldo_wif_fuse_bytes_fwd_dt
    err = lib.waldo_last_error_string
    assert fwd(16, 16, 16, 1, 4, 4, 4, 64, 1, -1.0, 2.0, TRUNC, NCHW, None) == -1 and b"bad shape" in err()  # C < 5
    assert fwd(16, 16, 16, 1, 4, 5, 3, 64, 1, -1.0, 2.0, TRUNC, NCHW, None) == -1 and b"bad shape" in err()  # Co < 4
    assert fwd(16, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, 2.0, NONE, NCHW, None) == -1 and b"quantisation" in err()
    assert fwd(16, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, 2.0, TRUNC, 2, None) == -1 and b"layout" in err()
    assert fwd(16, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, 0.0, TRUNC, NCHW, None) == -1 and b"bad span" in err()
    assert fwd(16, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, float("inf"), TRUNC, NCHW, None) == -1 and b"bad span" in err()
    assert fwd(None, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, 2.0, TRUNC, NCHW, None) == -1 and b"null pointer" in err()
    assert fwd(16, 16, None, 1, 4, 5, 4, 64, 1, -1.0, 2.0, TRUNC, NCHW, None) == -1 and b"null pointer" in err()
    assert fwd(16, 16, 16, 2 ** 31, 4, 5, 4, 4, 1, -1.0, 2.0, TRUNC, NCHW, None) == -1 and b"bad shape" in err()
    assert dt(16, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, 2.0, TRUNC, NCHW, 3, F32, None) == -1 and b"unknown dtype" in err()
    assert dt(16, 16, 16, 1, 4, 5, 4, 64, 1, -1.0, 2.0, TRUNC, NCHW, F32, 7, None) == -1 and b"unknown dtype" in err()


def test_header_has_a_byte_output_section_with_the_formula_and_the_nan_rule():
    text = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    start = text.index("Byte output:")
    sec = text[start:text.index("Reproducible gradients", start)]
    for needle in ("clamp((x - lo) / range, 0, 1)", "truncf(u * 255)", "truncf(u * 255 + 0.5)", "NaN", "byte 0",
                   "waldo_frames_to_bytes_fwd", "waldo_wif_fuse_bytes_fwd_dt"):
        assert needle in sec, needle


def test_both_units_use_the_one_quantisation_text():
    """quantize() of the scorer and the byte kernels call the same header's functions; the formula is written once."""
    csrc = os.path.join(ROOT, "waldo_amd", "csrc")
    hdr = open(os.path.join(csrc, "quantize.hip.h")).read()
    assert "(x - lo) / range" in hdr and "fminf(fmaxf(u, 0.0f), 1.0f)" in hdr
    for name in ("frame_metrics.hip", "frames_to_bytes.hip", "wif_fuse.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "quantize.hip.h"' in text, name
        assert "/ range" not in text and "* 255.0f" not in text, name
    # the renders take it through the row scheme's header; the formula is in neither
    rows, render = (open(os.path.join(csrc, name)).read() for name in ("byte_rows.hip.h", "render.hip"))
    assert '#include "quantize.hip.h"' in rows and '#include "byte_rows.hip.h"' in render
    for text in (rows, render):
        assert "/ range" not in text and "* 255.0f" not in text


def test_wrappers_have_no_cpu_fallback():
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    with pytest.raises(WaldoHipError):
        WF.frames_to_bytes(torch.zeros(2, 3, 4, 4))
    with pytest.raises(WaldoHipError):
        WF.frames_to_bytes(WF.PackedClip(torch.zeros(1, 2, 4, 4, 4, dtype=torch.uint8), 0))
    with pytest.raises(WaldoHipError):
        WF.wif_fuse_bytes(torch.zeros(1, 1, 2, 5, 4, 4), torch.zeros(1, 1, 2, 4, 4, 4))


def test_wrappers_refuse_unknown_names_and_shapes():
    from waldo_amd import functional as WF
    from waldo_amd.nets.wif import WIF
    from waldo_amd.tools import demo
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="quantize"):
        WF.frames_to_bytes(x, quantize="floor")
    with pytest.raises(ValueError, match="quantize"):
        WF.frames_to_bytes(x, quantize="none")
    with pytest.raises(ValueError, match="layout"):
        WF.frames_to_bytes(x, layout="hwc")
    with pytest.raises(ValueError, match="span"):
        WF.frames_to_bytes(x, span=(1.0, 1.0))
    with pytest.raises(ValueError, match="quantize"):
        WF.wif_fuse_bytes(torch.zeros(1, 1, 2, 5, 4, 4), torch.zeros(1, 1, 2, 4, 4, 4), quantize="floor")
    with pytest.raises(ValueError, match="layout"):
        WF.wif_fuse_bytes(torch.zeros(1, 1, 2, 5, 4, 4), torch.zeros(1, 1, 2, 4, 4, 4), layout="hwc")
    with pytest.raises(ValueError):
        WF.frames_to_bytes(torch.zeros(2, 3, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        WF.frames_to_bytes(torch.zeros(4, 4))
    wif = WIF(demo.demo_opt(dim=16))
    with pytest.raises(ValueError, match="out_bytes"):
        wif(torch.zeros(1, 2, 1, 5, 4, 4), out_bytes="floor")
    with pytest.raises(ValueError, match="out_bytes"):
        demo.predict(None, None, None, torch.zeros(1, 6, 3, 4, 4), None, None, 4, out_bytes="floor")
    with pytest.raises(ValueError, match="out_bytes"):
        demo.predict_sharded(demo.demo_opt(dim=16), None, None, torch.zeros(1, 6, 3, 4, 4), None, None, 4, 0, 2,
                             out_bytes="floor")
    with pytest.raises(ValueError, match="out_bytes"):
        demo.units_to_clips("rec_vid", torch.zeros(6, 3, 4, 4, dtype=torch.uint8), 1, 6, 4, 1, out_bytes="floor")


def test_binding_declares_the_entry_points():
    from waldo_amd import _lib
    sig = _lib.SIGNATURES
    assert sig["waldo_frames_to_bytes_fwd"][-1] is ctypes.c_void_p and len(sig["waldo_frames_to_bytes_fwd"]) == 17
    assert sig["waldo_wif_fuse_bytes_fwd_dt"] == sig["waldo_wif_fuse_bytes_fwd"][:-1] + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    assert "waldo_wif_fuse_bytes_bwd" not in sig  # forward only


def _byte_clip(t=3, h=6, w=8, channels=3, seed=0):
    """A uint8 clip with at most 256 colours per frame and over the clip (a GIF holds it exactly): every pixel one of 200
    random colours."""
    g = torch.Generator().manual_seed(seed)
    palette = torch.randint(0, 256, (200, channels), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, 200, (t, h, w), generator=g)
    return palette[idx].permute(0, 3, 1, 2).contiguous()  # (T, C, H, W)


@pytest.mark.parametrize("form", ["dir", "clip.png", "clip.gif"])
def test_dump_video_writes_a_uint8_clip_as_it_is(tmp_path, form):
    from waldo_amd.tools import io as wio
    clip = _byte_clip()
    path = str(tmp_path / form)
    if form == "dir":
        os.makedirs(path)
    wio.dump_video(clip, path)
    assert torch.equal(wio.load_video_u8(path), clip)
    # (T, H, W, 3), what frames_to_bytes(layout="nhwc") returns: the same file contents
    other = str(tmp_path / ("nhwc_" + form))
    if form == "dir":
        os.makedirs(other)
    wio.dump_video(clip.permute(0, 2, 3, 1).contiguous(), other)
    assert torch.equal(wio.load_video_u8(other), clip)


def test_dump_video_repeats_a_one_channel_clip(tmp_path):
    from waldo_amd.tools import io as wio
    clip = _byte_clip(channels=1)
    wio.dump_video(clip, str(tmp_path / "d"))
    assert torch.equal(wio.load_video_u8(str(tmp_path / "d")), clip.expand(-1, 3, -1, -1))


def test_dump_image_writes_uint8_as_it_is(tmp_path):
    import numpy as np
    import PIL.Image
    from waldo_amd.tools import io as wio
    img = _byte_clip(t=1)[0]
    for name, x in (("chw.png", img), ("hwc.png", img.permute(1, 2, 0).contiguous())):
        wio.dump_image(x, str(tmp_path / name))
        back = torch.from_numpy(np.asarray(PIL.Image.open(str(tmp_path / name)).convert("RGB")).copy())
        assert torch.equal(back.permute(2, 0, 1), img), name


def test_float_input_is_written_as_before(tmp_path):
    """Float clips still go through the span and the "round" quantisation: the files hold (u * 255 + 0.5) bytes."""
    from waldo_amd.tools import io as wio
    g = torch.Generator().manual_seed(1)
    clip = torch.rand(3, 3, 6, 8, generator=g) * 2.4 - 1.2
    want = (((clip - -1.0) / 2.0).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)
    wio.dump_video(clip, str(tmp_path / "f"))
    assert torch.equal(wio.load_video_u8(str(tmp_path / "f")), want)
    wio.dump_video(clip, str(tmp_path / "g"), span=(0.0, 1.0))
    assert torch.equal(wio.load_video_u8(str(tmp_path / "g")),
                       (clip.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8))
    wio.dump_image(clip[0], str(tmp_path / "i.png"))
    assert torch.equal(wio.load_video_u8(str(tmp_path / "i.png"))[0], want[0])


def test_trunc_does_not_give_a_packed_clips_bytes_back():
    """The round trip byte -> read_rgb's normalisation -> "trunc" is not the identity for 63 of the 256 byte values (and
    "round" is, for all of them): the context frames of a byte result are quantised, never copied.  The positions are what
    the device table of frames_to_bytes holds (tests/test_gpu_bytes.py compares it with this expression)."""
    from waldo_amd.tools.io import rgb_from_u8
    b = torch.arange(256, dtype=torch.uint8)
    x = rgb_from_u8(b)
    u = (x.clamp(-1.0, 1.0) - -1.0) / 2.0
    trunc, rnd = (u * 255).to(torch.uint8), (u * 255 + 0.5).to(torch.uint8)
    assert int((trunc != b).sum()) == 63
    assert torch.equal(rnd, b)
    off = (trunc != b).nonzero().flatten()
    assert torch.equal(trunc[off].int(), b[off].int() - 1)  # always one below
