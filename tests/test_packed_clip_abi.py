"""CPU: the packed clip (functional.PackedClip: RGB bytes + class id per pixel) -- its C ABI, the host-side validation of
its entry points, and its unpacked form against the fp32 clip the loader builds.  No compute call is made here."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "waldo_hip.h")
CLIP = os.path.join(ROOT, "tests", "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")
NEW = ("waldo_unpack_clip_fwd", "waldo_downscale_frames_packed_fwd", "waldo_flow_ctx_alpha_packed_fwd",
       "waldo_frame_warp_fuse_raw_packed_fwd")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def unpacked_reference(clip):
    """The unpacked form restated in torch: channels 0-2 read_rgb's normalisation of the RGB bytes, channel 3 + n
    +5 where the class id is n and -5 elsewhere."""
    from waldo_amd.tools import io
    d = clip.data.cpu()
    rgb = io.rgb_from_u8(d[..., :3]).permute(0, 1, 4, 2, 3)
    n = torch.arange(clip.num_lyt).view(1, 1, -1, 1, 1)
    lyt = torch.where(d[..., 3].long().unsqueeze(2) == n, 5.0, -5.0)
    return torch.cat([rgb, lyt], dim=2)


def test_packed_entry_points_declared_exported_and_bound(lib):
    from waldo_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(build.LIB)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION


def test_host_validation_without_gpu(lib):
    """A null clip, Nl = 33 and an unknown raw dtype: WALDO_EINVAL with a message, before any launch."""
    def err():
        return lib.waldo_last_error_string()

    # frame warp: clip, rgb_table, flow, score, ctx_ts, out, raw, status | B T Tc Tp Nl L Hd Wd include_self | eps dtype
    shape = [1, 4, 4, 1, 20, 8, 32, 32, 0]
    assert lib.waldo_frame_warp_fuse_raw_packed_fwd(*([None] * 8), *shape, 1e-6, 0, None) == -1
    assert b"null pointer" in err()
    bad = shape[:4] + [33] + shape[5:]
    assert lib.waldo_frame_warp_fuse_raw_packed_fwd(*([None] * 8), *bad, 1e-6, 0, None) == -1
    assert b"33 classes" in err()
    for code in (-1, 3, 9):
        assert lib.waldo_frame_warp_fuse_raw_packed_fwd(*([None] * 8), *shape, 1e-6, code, None) == -1
        assert b"unknown raw dtype" in err()
    # flow_ctx_alpha: alpha_lr, clip, dist, occ, a01, alpha_out, layer_bits | B T Tw L Nl H W scale
    assert lib.waldo_flow_ctx_alpha_packed_fwd(*([None] * 7), 1, 4, 4, 8, 20, 8, 8, 4, None) == -1
    assert b"null pointer" in err()
    assert lib.waldo_flow_ctx_alpha_packed_fwd(*([None] * 7), 1, 4, 4, 8, 33, 8, 8, 4, None) == -1
    assert b"33 classes" in err()
    # downscale: clip, out | B T Tw Nl H W S
    assert lib.waldo_downscale_frames_packed_fwd(None, None, 1, 4, 4, 20, 8, 8, 4, None) == -1
    assert b"null pointer" in err()
    assert lib.waldo_downscale_frames_packed_fwd(None, None, 1, 4, 4, 33, 8, 8, 4, None) == -1
    assert b"Nl=33" in err()
    # unpack: clip, rgb_table, out | B T Nl Hd Wd
    assert lib.waldo_unpack_clip_fwd(None, None, None, 1, 4, 20, 8, 8, None) == -1
    assert b"null pointer" in err()
    assert lib.waldo_unpack_clip_fwd(None, None, None, 1, 4, 33, 8, 8, None) == -1
    assert b"Nl=33" in err()
    assert lib.waldo_unpack_clip_fwd(None, None, None, 0, 4, 20, 8, 8, None) == 0  # nothing to do


@pytest.mark.parametrize("size", [None, (64, 128), (37, 61)])
def test_packed_load_clip_stands_for_the_fp32_clip(size):
    """The torch restatement of load_clip(packed=True)'s unpacked form == cat([vid, lyt], dim=1) of load_clip(), bit for
    bit, at the files' resolution and resized (bilinear RGB, nearest layout)."""
    from waldo_amd import functional as WF
    from waldo_amd.tools import io
    ref = io.load_clip(CLIP, size, 20)
    got = io.load_clip(CLIP, size, 20, packed=True)
    assert isinstance(got["vid"], WF.PackedClip) and got["lyt"] is None and got["names"] == ref["names"]
    want = torch.cat([ref["vid"], ref["lyt"]], dim=1).unsqueeze(0)
    assert tuple(got["vid"].shape) == tuple(want.shape)
    assert torch.equal(unpacked_reference(got["vid"]), want)


@pytest.mark.parametrize("src,dst", [((16, 24), (37, 61)), ((37, 61), (16, 24)), ((20, 30), (40, 60)),
                                     ((33, 47), (33, 47)), ((64, 128), (31, 65))])
def test_nearest_class_map_equals_nearest_one_hot(src, dst):
    """Nearest-resizing the class map == nearest-resizing its one-hot planes (what read_layout does), at up- and
    down-scaling and odd ratios."""
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    nl = 20
    cm = torch.randint(0, nl, src, generator=g)
    onehot = torch.zeros(nl, *src).scatter_(0, cm.unsqueeze(0), 1)
    planes = F.interpolate(onehot.unsqueeze(0), size=dst, mode="nearest")[0]
    ids = F.interpolate(cm[None, None].float(), size=dst, mode="nearest")[0, 0].long()
    assert torch.equal(torch.zeros(nl, *dst).scatter_(0, ids.unsqueeze(0), 1), planes)


def test_out_of_range_class_ids_refused(tmp_path):
    import numpy as np
    import PIL.Image
    from waldo_amd.tools import io
    p = os.path.join(tmp_path, "cm.png")
    PIL.Image.fromarray(np.full((8, 8), 21, np.uint8)).save(p)
    with pytest.raises(ValueError, match="class id 21"):
        io.read_class_map(p, 20)
    with pytest.raises(ValueError, match="class id 21"):
        io.read_layout(p, 20)


def test_packed_clip_type_on_the_host():
    """PackedClip: the unpacked form's shape, batch / time slices as views, fp32 new_empty; pack_clip's layout."""
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (2, 5, 3, 6, 10), generator=g, dtype=torch.uint8)
    cls = torch.randint(0, 25, (2, 5, 6, 10), generator=g)
    clip = WF.pack_clip(rgb, cls, 20)
    assert clip.shape == torch.Size((2, 5, 23, 6, 10)) and clip.size(2) == 23 and clip.size() == clip.shape
    assert clip.data.shape == (2, 5, 6, 10, 4) and clip.data.dtype == torch.uint8
    assert torch.equal(clip.data[..., :3], rgb.permute(0, 1, 3, 4, 2)) and torch.equal(clip.data[..., 3], cls.byte())
    part = clip[1:, 2:4]
    assert part.shape == torch.Size((1, 2, 23, 6, 10)) and part.data.data_ptr() == clip.data[1:, 2:4].data_ptr()
    assert clip[:, :3].size(1) == 3 and clip[:1].size(0) == 1
    with pytest.raises(IndexError):
        clip[:, :, 3:]
    e = clip.new_empty(3, 4)
    assert e.dtype == torch.float32 and e.shape == (3, 4) and not clip.requires_grad
    assert torch.equal(unpacked_reference(clip)[:, :, 3:].argmax(dim=2)[cls < 20], cls[cls < 20])
    assert (unpacked_reference(clip)[:, :, 3:][(cls >= 20).unsqueeze(2).expand(-1, -1, 20, -1, -1)] == -5).all()
    with pytest.raises(ValueError):
        WF.PackedClip(clip.data, 33)
    with pytest.raises(ValueError):
        WF.pack_clip(rgb, cls + 250, 20)
    assert torch.equal(WF.rgb_table("cpu"), (torch.arange(256).float() / 255.0 - 0.5) / 0.5)
