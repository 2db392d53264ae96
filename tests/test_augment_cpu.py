"""CPU: the clip augmentation (waldo_amd.augment, include/waldo_hip.h "Clip augmentation") without a GPU -- the
parameters against the reference's arithmetic in plain Python, every host-side refusal of the Python interface and of
the C ABI, and the restatement the GPU tests compare with (tests/augment_ref.py) against PIL's bytes
(tests/golden/augment_pil.npz, tools_dev/make_augment_golden.py) and against F.interpolate."""
import math
import os
import types

import numpy as np
import PIL.Image
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = os.path.join(ROOT, "tests", "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")
FIXTURE = os.path.join(ROOT, "tests", "golden", "augment_pil.npz")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


# --------------------------------------------------------------------------------------
# parameters
# --------------------------------------------------------------------------------------
CITYSCAPES = dict(size=(128, 256), aspect_ratio=2.0, true_ratio=2.0, max_zoom=1.3)
KITTI_LIKE = dict(size=(128, 384), aspect_ratio=3.25, true_ratio=3.0, max_zoom=1.3)  # aspect_ratio / true_ratio > 1


def edge_uniforms(fields):
    """Rows of eight uniforms: 0, just under 1, the middle, and around every zoom at which h / zoom is an integer."""
    h = fields["size"][0]
    min_zoom = max(1.0, fields["aspect_ratio"] / fields["true_ratio"])
    top_zoom = max(fields["max_zoom"], min_zoom)
    under_one = math.nextafter(1.0, 0.0)
    zooms = [0.0, under_one, 0.5]
    for k in range(int(h / top_zoom), int(h / min_zoom) + 1):  # h / zoom == k
        uz = (h / k - min_zoom) / (top_zoom - min_zoom)
        zooms += [v for v in (math.nextafter(uz, 0.0), uz, math.nextafter(uz, 1.0)) if 0.0 <= v < 1.0]
    others = [0.0, under_one, 0.5, 0.25, 0.75, math.nextafter(0.5, 1.0), 0.123456789, 0.987654321]
    rows = []
    for i, uz in enumerate(zooms):
        row = [others[(i + 3 * c) % len(others)] for c in range(8)]
        row[2] = uz
        rows.append(row)
    for v in (0.0, under_one):  # every column at the same end
        rows.append([v] * 8)
    return rows


@pytest.mark.parametrize("fields", [CITYSCAPES, KITTI_LIKE], ids=["cityscapes", "kitti_like"])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("colorjitter", [0.5, None])
def test_params_equal_the_reference_arithmetic(fields, train, colorjitter):
    """params_from_uniforms == get_augmentation_parameters' default branch in Python floats: boxes and flips as
    integers, jitter and zoom as the fp32 of the same fp64 numbers."""
    from waldo_amd import augment as A
    rows = edge_uniforms(fields)
    t = 3
    u = torch.tensor(rows, dtype=torch.float64)
    u_order = (torch.arange(len(rows) * t).view(-1, t) * 5) % 6
    got = A.params_from_uniforms(u, u_order, lr_flip=True, tb_flip=True, colorjitter=colorjitter, train=train, **fields)
    assert got.box.dtype == torch.int32 and got.flip.dtype == torch.uint8 and got.order.dtype == torch.uint8
    assert got.jitter.dtype == torch.float32 and got.zoom.dtype == torch.float32
    h, w = fields["size"]
    landed = 0
    for i, row in enumerate(rows):
        flip, box, jitter, zoom = R.reference_parameters(
            row, h=h, w=w, aspect_ratio=fields["aspect_ratio"], true_ratio=fields["true_ratio"],
            max_zoom=fields["max_zoom"], lr_flip=True, tb_flip=True, colorjitter=colorjitter, train=train)
        assert got.box[i].tolist() == box, (i, row)
        assert int(got.flip[i]) == flip, (i, row)
        assert got.zoom[i].item() == np.float32(zoom), (i, row)
        landed += float(h / zoom).is_integer()
        if jitter is None:
            assert got.jitter[i].tolist() == [1.0, 1.0, 0.0] and (got.order[i] == 255).all()
        else:
            assert got.jitter[i].tolist() == [float(np.float32(v)) for v in jitter], (i, row)
            assert torch.equal(got.order[i].long(), u_order[i])
    A.check_params(got, (len(rows), t, 23, h, w))
    if train:
        assert landed >= 3  # (the rows built around integer h / zoom do hit it)
    else:
        min_zoom = max(1.0, fields["aspect_ratio"] / fields["true_ratio"])
        assert (got.box[:, :2] == 0).all() and (got.flip == 0).all() and (got.order == 255).all()
        assert (got.box[:, 2] == int(h / min_zoom)).all()


def test_flips_are_drawn_only_where_offered():
    from waldo_amd import augment as A
    u = torch.full((4, 8), 0.9, dtype=torch.float64)
    o = torch.zeros(4, 2, dtype=torch.long)
    for lr, tb, want in ((False, False, 0), (True, False, 1), (False, True, 2), (True, True, 3)):
        p = A.params_from_uniforms(u, o, lr_flip=lr, tb_flip=tb, **CITYSCAPES)
        assert (p.flip == want).all()
    with pytest.raises(ValueError, match=r"\(B, 8\)"):
        A.params_from_uniforms(u[:, :7], o, **CITYSCAPES)


def test_sample_params_distributions_and_seed():
    from waldo_amd import augment as A
    kw = dict(lr_flip=True, tb_flip=False, colorjitter=0.5, device="cpu", **CITYSCAPES)
    a = A.sample_params(512, 4, generator=torch.Generator().manual_seed(3), **kw)
    b = A.sample_params(512, 4, generator=torch.Generator().manual_seed(3), **kw)
    for x, y in zip(a.tensors().values(), b.tensors().values()):
        assert torch.equal(x, y)
    A.check_params(a, (512, 4, 23, 128, 256))
    assert 1.0 <= a.zoom.min() and a.zoom.max() < 1.3 and 1.1 < a.zoom.mean() < 1.2
    assert set(a.flip.tolist()) == {0, 1} and set(a.order.unique().tolist()) == set(range(6))
    assert 0.5 <= a.jitter[:, :2].min() and a.jitter[:, :2].max() <= 1.5 and a.jitter[:, 2].abs().max() <= 0.25


# --------------------------------------------------------------------------------------
# refusals of the Python interface
# --------------------------------------------------------------------------------------
def good_params(b=2, t=3):
    from waldo_amd import augment as A
    return A.AugmentParams(torch.tensor([[0, 0, 20, 68], [7, 41, 13, 27]], dtype=torch.int32)[:b],
                           torch.zeros(b, dtype=torch.uint8), torch.tensor([[1.0, 1.0, 0.0]] * b),
                           torch.full((b, t), 255, dtype=torch.uint8), torch.ones(b))


@pytest.mark.parametrize("name,value,match", [
    ("box", torch.tensor([[0, 0, 20, 68], [8, 41, 13, 27]], dtype=torch.int32), "does not lie inside"),   # bottom edge
    ("box", torch.tensor([[0, 0, 20, 68], [7, 42, 13, 27]], dtype=torch.int32), "does not lie inside"),   # right edge
    ("box", torch.tensor([[-1, 0, 20, 68], [7, 41, 13, 27]], dtype=torch.int32), "does not lie inside"),
    ("box", torch.tensor([[0, 0, 0, 68], [7, 41, 13, 27]], dtype=torch.int32), "does not lie inside"),
    ("box", torch.tensor([[0, 0, 20, 68]], dtype=torch.int32), "box must be"),
    ("box", torch.tensor([[0, 0, 20, 68], [7, 41, 13, 27]]), "box must be"),                             # int64
    ("flip", torch.tensor([0, 4], dtype=torch.uint8), "flip holds bits"),
    ("order", torch.tensor([[0, 5, 255], [6, 0, 0]], dtype=torch.uint8), "order holds a byte"),
    ("order", torch.zeros(2, 4, dtype=torch.uint8), "order must be"),
    ("jitter", torch.tensor([[1.0, 1.0, 0.0], [-0.1, 1.0, 0.0]]), "jitter must be finite"),
    ("jitter", torch.tensor([[1.0, 1.0, 0.6], [1.0, 1.0, 0.0]]), "jitter must be finite"),
    ("jitter", torch.tensor([[1.0, float("nan"), 0.0], [1.0, 1.0, 0.0]]), "jitter must be finite"),
    ("zoom", torch.tensor([1.0, 0.0]), "zoom must be finite"),
    ("zoom", torch.tensor([1.0, float("inf")]), "zoom must be finite"),
])
def test_check_params_refusals(name, value, match):
    from waldo_amd import augment as A
    p = good_params()
    A.check_params(p, (2, 3, 8, 20, 68))
    setattr(p, name, value)
    with pytest.raises(ValueError, match=match):
        A.check_params(p, (2, 3, 8, 20, 68))


def recipe_opt(**over):
    opt = types.SimpleNamespace(max_zoom=1.3, no_v_flip=False, no_h_flip=True, colorjitter=0.5,
                                colorjitter_no_contrast=True, aspect_ratio=2.0, true_ratio=2.0, dim=128, load_dim=0,
                                true_dim=128, rotate=0, fixed_crop=None, fixed_top_centered_zoom=None)
    vars(opt).update(over)
    return opt


def test_from_opt_reads_the_recipe_options():
    from waldo_amd import augment as A
    a = A.Augmenter.from_opt(recipe_opt())
    assert (a.size, a.clip_size, a.max_zoom, a.lr_flip, a.tb_flip, a.colorjitter) == ((128, 256), (128, 256), 1.3, True,
                                                                                      False, 0.5)
    a = A.Augmenter.from_opt(recipe_opt(dim=128, load_dim=512, true_dim=512, colorjitter=None,
                                        colorjitter_no_contrast=False, no_v_flip=True, no_h_flip=False))
    assert (a.size, a.clip_size, a.lr_flip, a.tb_flip, a.colorjitter) == ((512, 1024), (512, 1024), False, True, None)
    a = A.Augmenter.from_opt(recipe_opt(aspect_ratio=3.25, true_ratio=3.0))
    assert (a.size, a.clip_size) == ((128, 416), (128, 384))


@pytest.mark.parametrize("over,field", [
    (dict(rotate=0.1), "rotate"), (dict(fixed_crop=[64, 128]), "fixed_crop"),
    (dict(fixed_top_centered_zoom=1.5), "fixed_top_centered_zoom"),
    (dict(colorjitter_no_contrast=False), "colorjitter_no_contrast"),
    (dict(true_dim=256), "true_dim"), (dict(load_dim=512, true_dim=128), "true_dim")])
def test_from_opt_refusals_name_the_field(over, field):
    from waldo_amd import augment as A
    with pytest.raises(ValueError, match=field):
        A.Augmenter.from_opt(recipe_opt(**over))


def test_augment_clip_refusals_on_the_host():
    """A CPU clip: WaldoHipError (no CPU fallback), like unpack_clip; bad arguments: ValueError before the device matters."""
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    clip = WF.PackedClip(torch.zeros(2, 3, 20, 68, 4, dtype=torch.uint8), 5)
    with pytest.raises(WaldoHipError, match="no CPU"):
        A.augment_clip(clip, good_params())
    with pytest.raises(ValueError, match="PackedClip"):
        A.augment_clip(clip.data, good_params())
    a = A.Augmenter(size=(20, 68), clip_size=(128, 256))
    with pytest.raises(ValueError, match="the options say"):
        a.params(clip)


# --------------------------------------------------------------------------------------
# the C ABI without a GPU
# --------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound(lib):
    from waldo_amd import _lib
    assert hasattr(lib, "waldo_augment_clip_fwd") and "waldo_augment_clip_fwd" in _lib.SIGNATURES
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION


def test_host_validation_without_gpu(lib):
    """Every WALDO_EINVAL of the header, with its message, before any launch; B T == 0: WALDO_OK."""
    P = 0x1000  # a non-null address that is never dereferenced: every call below returns before a launch

    def call(ptrs=None, flow=(None, None), B=2, T=3, Nl=5, Hd=20, Wd=68, Hf=8, Wf=27, Ho=23, Wo=70):
        clip, box, flip, jitter, order, zoom, out = ptrs or [None] * 7  # (the shape refusals come before the pointers)
        rc = lib.waldo_augment_clip_fwd(clip, flow[0], box, flip, jitter, order, zoom, out, flow[1], B, T, Nl, Hd, Wd,
                                        Hf, Wf, Ho, Wo, None)
        return rc, lib.waldo_last_error_string()

    for kw in (dict(Ho=19), dict(Wo=67)):
        rc, msg = call(**kw)
        assert rc == -1 and b"downsample" in msg, (kw, msg)
    for kw in (dict(Hf=21), dict(Wf=69)):
        rc, msg = call(flow=(P, None), **kw)
        assert rc == -1 and b"flow larger than the clip" in msg, (kw, msg)
    for kw in (dict(Nl=33), dict(Nl=-1), dict(B=-1), dict(T=-1), dict(Hd=0), dict(Wd=0), dict(Hd=32768, Ho=32768),
               dict(Wd=32768, Wo=32768), dict(Ho=32768), dict(Wo=32768), dict(Ho=0), dict(Wo=0)):
        rc, msg = call(**kw)
        assert rc == -1 and b"bad shape" in msg, (kw, msg)
    for kw in (dict(Hf=0), dict(Wf=0), dict(Hf=32768), dict(Wf=-3)):
        rc, msg = call(flow=(None, P), **kw)
        assert rc == -1 and b"bad shape" in msg, (kw, msg)
    for k in range(7):  # clip, box, flip, jitter, order, zoom, out
        ptrs = [P] * 7
        ptrs[k] = None
        rc, msg = call(ptrs=ptrs)
        assert rc == -1 and b"null pointer" in msg, (k, msg)
    for flow in ((P, None), (None, P)):  # flow and flow_out are null together or not at all
        rc, msg = call(ptrs=[P] * 7, flow=flow)
        assert rc == -1 and b"null pointer" in msg, (flow, msg)
    # more than 2^31 - 1 workgroups: 32767 x 32767 pixels, one per lane (Wo % 4 != 0), 256 per workgroup, 520 frames
    rc, msg = call(ptrs=[P] * 7, B=65, T=8, Hd=1, Wd=1, Ho=32767, Wo=32767)
    assert rc == -1 and b"too large" in msg, msg
    # nothing to do: WALDO_OK without a launch, whatever the pointers
    assert call(B=0)[0] == 0
    assert call(T=0)[0] == 0
    assert call(B=0, Ho=19)[0] == -1  # (a bad shape is refused first)


# --------------------------------------------------------------------------------------
# the restatement: against F.interpolate, and against PIL's bytes
# --------------------------------------------------------------------------------------
def test_restatement_resize_is_f_interpolate():
    """The crop + resize of the restatement == F.interpolate(bilinear, align_corners=False) on the cropped planes, for
    RGB, the one-hot layout and both resizes of the flow (fp64: both evaluate the same expression)."""
    g = torch.Generator().manual_seed(5)
    hd, wd, nl = 20, 68, 5
    data = torch.randint(0, 256, (1, 2, hd, wd, 4), generator=g, dtype=torch.uint8)
    data[..., 3] = torch.randint(0, nl + 2, (1, 2, hd, wd), generator=g)
    flow = torch.randn(1, 2, 2, 8, 27, generator=g)
    top, left, hc, wc = 7, 41, 13, 27
    p = types.SimpleNamespace(box=torch.tensor([[top, left, hc, wc]]), flip=torch.zeros(1, dtype=torch.uint8),
                              jitter=torch.tensor([[1.0, 1.0, 0.0]]), order=torch.full((1, 2), 255), zoom=torch.ones(1))
    out, fl = R.augment_ref(data, nl, p, flow=flow, out_size=(23, 70), dtype=torch.float64)
    crop = data[0, :, top:top + hc, left:left + wc].double()
    rgb = F.interpolate(crop[..., :3].permute(0, 3, 1, 2) / 255, size=(23, 70), mode="bilinear", align_corners=False)
    assert (out[0, :, :3] - (rgb - 0.5) / 0.5).abs().max() < 1e-12
    onehot = (crop[..., 3].long().unsqueeze(1) == torch.arange(nl).view(1, -1, 1, 1)).double()
    lyt = F.interpolate(onehot, size=(23, 70), mode="bilinear", align_corners=False)
    assert (out[0, :, 3:] - 5 * (2 * lyt - 1)).abs().max() < 1e-12
    full = F.interpolate(flow[0].double(), size=(hd, wd), mode="bilinear", align_corners=False)
    want = F.interpolate(full[:, :, top:top + hc, left:left + wc], size=(23, 70), mode="bilinear", align_corners=False)
    assert (fl[0] - want).abs().max() < 1e-12


@pytest.fixture(scope="module")
def fixture_gap():
    """|restatement (fp64) - PIL| in bytes, per draw: (D, 2, 3, h, w) over the fixture's stored region."""
    g = np.load(FIXTURE)
    frames = np.stack([np.asarray(PIL.Image.open(os.path.join(FRAMES, str(n))).convert("RGB")) for n in g["names"]])
    d = len(g["box"])
    data = torch.from_numpy(frames)[None].expand(d, -1, -1, -1, -1)
    data = torch.cat([data, torch.zeros(*data.shape[:4], 1, dtype=torch.uint8)], dim=-1).contiguous()
    p = types.SimpleNamespace(box=torch.from_numpy(g["box"]), flip=torch.from_numpy(g["flip"]),
                              jitter=torch.from_numpy(g["jitter"]), order=torch.from_numpy(g["order"]), zoom=torch.ones(d))
    out, _ = R.augment_ref(data, 0, p, out_size=tuple(int(v) for v in g["size"]), dtype=torch.float64)
    t0, l0, rh, rw = (int(v) for v in g["region"])
    got = (out[:, :, :3, t0:t0 + rh, l0:l0 + rw] * 0.5 + 0.5) * 255
    gap = (got - torch.from_numpy(g["rgb"]).permute(0, 1, 4, 2, 3).double()).abs()
    jittered = torch.from_numpy(g["order"] != 255)  # (D, 2)
    return gap, jittered, int(g["resize_only"])


def test_restatement_against_pil_without_jitter(fixture_gap):
    """Crop + bilinear resize (+ flips) alone: within 1 byte of PIL, which rounds to 8 bits once after each of its two
    passes (0.5 + 0.5).  The resize-only draw and the two sampled draws without jitter."""
    gap, jittered, resize_only = fixture_gap
    assert not jittered[resize_only].any()
    plain = gap[~jittered]
    print(f"[augment] no jitter: max gap {plain.max():.3f} / 255, mean {plain.mean():.3f} / 255 "
          f"(resize-only draw: max {gap[resize_only].max():.3f})")
    assert gap[resize_only].max() <= 1.0
    assert plain.max() <= 1.0


def test_restatement_against_pil_with_jitter(fixture_gap):
    """The jittered draws at colorjitter 0.5.  PIL rounds to 8 bits after the resize and after every jitter operation
    and shifts the hue in an 8-bit HSV; the float route does neither.  Measured when the fixture was made, over its six
    jittered draws x two frames: max gap 5.27 / 255, mean at most 1.10 / 255 per draw (5.27, 4.39, 4.13, 2.95, 3.11, 4.57
    max; 1.10, 1.02, 1.00, 0.85, 0.96, 0.90 mean).  The bounds are those with a margin of 1.5: a formula error (wrong
    grey weights, a wrong hue sign) shows as tens of bytes, not as rounding."""
    gap, jittered, _ = fixture_gap
    assert int(jittered.sum()) == 12
    per_draw_max = gap.amax(dim=(1, 2, 3, 4))
    per_draw_mean = gap.mean(dim=(1, 2, 3, 4))
    print("[augment] jitter: max gap per draw", [round(float(v), 3) for v in per_draw_max],
          "mean", [round(float(v), 3) for v in per_draw_mean])
    assert gap[jittered].max() <= 1.5 * 5.27
    assert per_draw_mean[jittered.any(dim=1)].max() <= 1.5 * 1.10
