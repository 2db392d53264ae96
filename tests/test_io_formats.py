"""Row f4: on-disk formats of the demo clips (host logic; no GPU)."""
import os

import numpy as np
import pytest
import torch

from waldo_amd.tools import io as wio

HERE = os.path.dirname(os.path.abspath(__file__))
DEMO = os.path.join(HERE, "golden", "demo_flow.flo")  # a data file of the reference's demo set


def test_read_flo_demo_file():
    flow = wio.read_flo(DEMO)
    assert flow.shape == (2, 128, 256) and flow.dtype == torch.float32
    raw = wio.read_flo(DEMO, normalize=False)
    assert torch.equal(flow[0], 2.0 * raw[0] / 256) and torch.equal(flow[1], 2.0 * raw[1] / 128)
    assert torch.isfinite(flow).all() and flow.abs().max() < 2.0


def test_flo_round_trip_and_errors(tmp_path):
    g = torch.Generator().manual_seed(0)
    flow = torch.randn(2, 7, 11, generator=g)
    p = tmp_path / "a.flo"
    wio.write_flo(p, flow)
    back = wio.read_flo(p)
    assert torch.allclose(back, flow, atol=1e-6)
    wio.write_flo(p, flow, normalized=False)
    assert torch.equal(wio.read_flo(p, normalize=False), flow)
    (tmp_path / "bad.flo").write_bytes(b"XXXX" + b"\0" * 16)
    with pytest.raises(ValueError):
        wio.read_flo(tmp_path / "bad.flo")
    data = open(p, "rb").read()
    (tmp_path / "short.flo").write_bytes(data[:-8])
    with pytest.raises(ValueError):
        wio.read_flo(tmp_path / "short.flo")


def test_layout_to_logits():
    cm = torch.tensor([[0, 1, 2], [2, 255, 1]])
    lg = wio.layout_to_logits(cm, 4, remap_lyt=(255, 3))
    assert lg.shape == (4, 2, 3)
    assert torch.equal(lg.argmax(0), torch.tensor([[0, 1, 2], [2, 3, 1]]))
    assert set(lg.unique().tolist()) == {-5.0, 5.0} and torch.equal((lg > 0).sum(0), torch.ones(2, 3, dtype=torch.long))


def test_formats_against_reference_loader():
    """The reference's own loader methods (data/base_dataset.py) on the committed demo files, recorded by
    oracle/make_golden.py:gen_io_formats as the SHA-256 of their float32 bytes: the product's readers give the same
    tensors bit for bit -- the flow file, the first layout map, the first frame at three sizes."""
    import hashlib
    ref = np.load(os.path.join(HERE, "golden", "io_formats_reference_loader.npz"))

    def check(key, t):
        t = t.contiguous()
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(ref[key + ".shape"]), (key, t.shape)
        assert hashlib.sha256(t.numpy().tobytes()).digest() == ref[key + ".sha256"].tobytes(), key

    check("flow", wio.read_flo(DEMO))
    clip = os.path.join(HERE, "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")
    lyt_dir = clip.replace("_512", "_deeplabv3_512")
    p = os.path.join(lyt_dir, sorted(os.listdir(lyt_dir))[0])
    import PIL.Image
    ids = torch.from_numpy(np.asarray(PIL.Image.open(p)).copy()).long()
    check("layout", wio.layout_to_logits(ids, 20))
    check("layout", wio.read_layout(p, 20))
    pi = os.path.join(clip, sorted(os.listdir(clip))[0])
    for dim, ar in ((128, 1.0), (128, 2.0), (512, 2.0)):
        check(f"rgb_{dim}_{int(dim * ar)}", wio.read_rgb(pi, (dim, int(dim * ar))))


CLIP = os.path.join(HERE, "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")


def test_load_clip_and_dumps(tmp_path):
    """The committed six-frame demo clip (C1) through load_clip, and the result writers."""
    import PIL.Image
    clip = wio.load_clip(CLIP, (64, 128), 20, max_frames=5)
    assert clip["vid"].shape == (5, 3, 64, 128) and clip["lyt"].shape == (5, 20, 64, 128)
    assert clip["flow"] is None and clip["names"][0].endswith("000001_leftImg8bit.png")
    assert clip["vid"].min() >= -1 and clip["vid"].max() <= 1 and clip["vid"].std() > 0.1
    assert torch.equal((clip["lyt"] > 0).sum(1), torch.ones(5, 64, 128, dtype=torch.long))
    wio.dump_image(clip["vid"][0], tmp_path / "f.png")
    back = wio.read_rgb(tmp_path / "f.png")
    assert (back - clip["vid"][0]).abs().max() <= 1.0 / 255 + 1e-6
    wio.dump_video(clip["vid"], str(tmp_path / "v.gif"))
    assert PIL.Image.open(tmp_path / "v.gif").n_frames == 5
    wio.dump_video(clip["vid"], str(tmp_path / "frames"))
    assert sorted(os.listdir(tmp_path / "frames")) == [f"{i:04d}.png" for i in range(5)]
    with pytest.raises(ValueError):
        wio.dump_video(clip["vid"], str(tmp_path / "v.mp4"))
    with pytest.raises(ValueError):
        wio.read_layout(os.path.join(CLIP.replace("_512", "_deeplabv3_512"), clip["names"][0]), 5)
