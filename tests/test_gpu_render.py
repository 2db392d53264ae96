"""GPU: the renders (waldo_amd.render: class_ids, render_argmax, render_flow; tools.demo.predict(render=...)).
Ids are compared bit for bit with torch.max's index on the CPU, palette renders bit for bit with what the reference's
Logger.get_lyt returned (tests/golden/render_reference.npz, tools_dev/make_render_golden.py), the flow render with the
reference's Logger.get_flow_rgb under the rule written at test_flow_against_the_reference."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CLASSES = [1, 2, 12, 20, 33]
# 5 x 37 and 3 x 129: dense rows merge into one of 185 / 387 pixels -- head, full 16-pixel groups and a 4 + 1 / 3 tail
# (and, as non-dense rows of 37 / 129, groups and a 4 + 1 / 1 tail per row); 12 x 20: no full group in a row; 3 x 1400:
# one row of 4200 pixels, past a workgroup's 4096 -- a second workgroup whose lanes hold a body and a 4 + 4 tail (and, as
# non-dense rows of 1400, 87 groups and an 8-pixel tail per row)
SIZES = [(5, 37), (12, 20), (3, 129), (3, 1400)]


@pytest.fixture(scope="module")
def fixture():
    data = np.load(os.path.join(ROOT, "tests", "golden", "render_reference.npz"))
    return {k: np.asarray(data[k]) for k in data.files}


def ref_ids(x):
    return x.float().cpu().max(dim=-3)[1].to(torch.uint8)


def class_frames(c, h, w, dtype, seed=0, extra=4, pad=0):
    """(2, 3, 3 + c + 1, h, w + pad) seeded values on a grid of 1 / 16 (exact in every dtype; equal maxima occur on their
    own) whose channel slice 3 : 3 + c holds the planted cases: ties, +-0, NaN in one and in two channels, +-inf, a
    constant frame."""
    g = torch.Generator().manual_seed(seed + 1000 * c + h)
    x = (torch.randn(2, 3, extra + c, h, w + pad, generator=g) * 24).round() / 16
    s = x[:, :, 3:3 + c]
    s[0, 0, :, 0, 0] = 0.25                      # all equal -> 0
    s[0, 0, :, 0, 1] = -1.0                      # -0.0 first, +0.0 last: equal -> the first
    s[0, 0, 0, 0, 1], s[0, 0, c - 1, 0, 1] = -0.0, 0.0
    s[0, 0, c - 1, 0, 2] = float("nan")          # one NaN beats everything
    s[0, 0, c // 2, 0, 3] = float("nan")         # two NaNs: the first
    s[0, 0, c - 1, 0, 3] = float("nan")
    s[0, 0, c - 1, 0, 4] = float("inf")
    s[0, 0, :, 0, 5] = float("-inf")             # all -inf -> 0 ...
    s[0, 0, c // 2, 0, 6] = float("inf")         # ... +inf twice: the first
    s[0, 0, c - 1, 0, 6] = float("inf")
    s[0, 1, :, h - 1, w - 1] = -2.0              # in the tail: two equal maxima, the lower channel wins
    s[0, 1, c // 2, h - 1, w - 1] = s[0, 1, c - 1, h - 1, w - 1] = 9.0
    s[0, 2, c - 1, 0, 7] = float("nan")          # NaN in the last channel, +inf before it
    s[0, 2, 0, 0, 7] = float("inf")
    s[1, 2] = 0.5                                # a constant frame
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("c", CLASSES)
def test_ids_equal_torch_max_on_every_source_layout(dev, c, hw, dtype):
    from waldo_amd import render as R
    h, w = hw
    full = class_frames(c, h, w, dtype).to(dev)
    x = full[:, :, 3:3 + c]                     # the channel slice, read in place
    want = ref_ids(x)
    got = R.class_ids(x)
    assert got.dtype == torch.uint8 and got.shape == (2, 3, h, w)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(R.class_ids(x[:, 1:]).cpu(), want[:, 1:])             # a time slice
    assert torch.equal(R.class_ids(x[1, 2]).cpu(), want[1, 2])               # one frame, no leading dimension
    wide = class_frames(c, h, w, dtype, pad=3).to(dev)[:, :, 3:3 + c, :, 1:1 + w]  # rows not dense: element loads
    assert torch.equal(R.class_ids(wide).cpu(), ref_ids(wide))
    # the three output modes agree, in both layouts
    pal = torch.from_numpy(np.random.default_rng(c).integers(0, 256, (c + 2, 3), dtype=np.uint8))
    want_rgb = pal[want.long()]                                              # (2, 3, h, w, 3)
    for layout in ("nchw", "nhwc"):
        expect = want_rgb if layout == "nhwc" else want_rgb.permute(0, 1, 4, 2, 3)
        rgb = R.render_argmax(x, pal, layout=layout)
        assert rgb.dtype == torch.uint8 and torch.equal(rgb.cpu(), expect), layout
        rgb2, ids2 = R.render_argmax(x, pal.to(dev), layout=layout, return_ids=True)
        assert torch.equal(rgb2, rgb) and torch.equal(ids2.cpu(), want), layout


def _guarded(shape, dev, offset=1):
    """A uint8 view of ``shape`` ``offset`` bytes into a larger buffer filled with 0xAB."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev)
    return buf, buf[offset:offset + n].view(shape)


def _guard_intact(buf, body, offset=1):
    n = body.numel()
    return bool((buf[:offset] == 0xAB).all()) and bool((buf[offset + n:] == 0xAB).all())


@pytest.mark.parametrize("offset", [1, 4, 13])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_out_views_at_any_alignment(dev, hw, offset):
    """``out=`` as a view ``offset`` bytes into a larger buffer: the same bytes as a fresh result, nothing around them
    touched -- for the ids, both RGB layouts and the flow render."""
    from waldo_amd import render as R
    h, w = hw
    c = 12
    x = class_frames(c, h, w, torch.float32).to(dev)[:, :, 3:3 + c]
    pal = R.layer_palette(c)
    buf, out = _guarded((2, 3, h, w), dev, offset)
    assert R.class_ids(x, out=out) is out
    assert torch.equal(out, R.class_ids(x)) and _guard_intact(buf, out, offset)
    flow = torch.randn(2, 3, 2, h, w, generator=torch.Generator().manual_seed(7)).to(dev) * 0.1
    for layout in ("nchw", "nhwc"):
        shape = (2, 3, h, w, 3) if layout == "nhwc" else (2, 3, 3, h, w)
        buf, out = _guarded(shape, dev, offset)
        assert R.render_argmax(x, pal, layout=layout, out=out) is out
        assert torch.equal(out, R.render_argmax(x, pal, layout=layout)) and _guard_intact(buf, out, offset), layout
        buf, out = _guarded(shape, dev, offset)
        assert R.render_flow(flow, layout=layout, out=out) is out
        assert torch.equal(out, R.render_flow(flow, layout=layout)) and _guard_intact(buf, out, offset), layout
    with pytest.raises(ValueError, match="dense frames"):
        R.class_ids(x, out=torch.empty(2, 3, h, w + 1, dtype=torch.uint8, device=dev)[..., :w])


def _bytes_of(lyt):
    """get_lyt's values ((byte / 255 - 0.5) / 0.5 in fp32) mapped back to the bytes."""
    return torch.from_numpy(np.round((lyt.astype(np.float64) * 0.5 + 0.5) * 255).astype(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_rgb_equals_the_references_get_lyt(dev, fixture, dtype):
    """Object layers through the jet colours (synthesizer.py:260, 397) and layout logits through the two dataset
    palettes (:261): bit for bit what Logger.get_lyt returned.  (The fixture's values are exact in bf16 and fp16.)"""
    from waldo_amd import render as R
    for L in (4, 17):
        alpha = torch.from_numpy(fixture[f"alpha{L}"]).to(dev, dtype)
        want = _bytes_of(fixture[f"lyt_alpha{L}"])
        assert torch.equal(R.render_argmax(alpha, R.layer_palette(L)).cpu(), want), L
        assert torch.equal(R.render_argmax(alpha, R.layer_palette(L), layout="nhwc").cpu(), want.permute(0, 1, 3, 4, 2)), L
    logits = torch.from_numpy(fixture["logits"]).to(dev, dtype)
    assert torch.equal(R.render_argmax(logits, R.layer_palette(20)).cpu(), _bytes_of(fixture["lyt_jet20"]))
    city, kitti = fixture["palette_cityscapes"], fixture["palette_kitti"]
    assert torch.equal(R.render_argmax(logits, R.semantic_palette(city)).cpu(), _bytes_of(fixture["lyt_cityscapes"]))
    assert torch.equal(R.render_argmax(logits[:, :, :19], R.semantic_palette(kitti)).cpu(), _bytes_of(fixture["lyt_kitti"]))


# ---------------------------------------------------------------------------------------------------------- flow
def _trunc_bytes(x):
    return (x.float().clamp(0, 1) * 255.0).to(torch.uint8)


def test_flow_against_the_reference(dev, fixture):
    """Against Logger.get_flow_rgb's bytes ("trunc").  Rule: every channel within 1 level, except at pixels where the
    reference's own theta * K lies within 1e-3 of an integer -- there the bin is unstable under a one-ulp change of atan2
    -- and those pixels are at most 2 % of the fixture (1.1 % are planted ON bin boundaries: zeros, axis-aligned and
    diagonal vectors; a random direction falls this close with probability 2e-3)."""
    from waldo_amd import render as R
    flow = torch.from_numpy(fixture["flow"])                       # (3, 24, 40, 2)
    want = _trunc_bytes(torch.from_numpy(fixture["flow_rgb"]))     # (3, 3, 24, 40)
    got = R.render_flow(flow.permute(0, 3, 1, 2).to(dev)).cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    theta = (1 + torch.atan2(flow[..., 1], flow[..., 0]) / np.pi) / 2   # (tools/logger.py:313, on the CPU)
    tk = theta * 128
    unstable = (tk - tk.round()).abs() < 1e-3
    share = unstable.float().mean().item()
    diff = (got.int() - want.int()).abs()
    print(f"flow render: {100 * (diff != 0).float().mean().item():.4f} % of the bytes differ from the reference's, "
          f"max {int(diff.max())} level(s); {100 * (diff != 0).any(dim=1).float().mean().item():.4f} % of the pixels; "
          f"unstable share {100 * share:.2f} %")
    assert share <= 0.02
    assert int(diff.amax(dim=1)[~unstable].max()) <= 1
    assert float(got.float().std()) > 20  # not a blank picture


def test_flow_exact_cases(dev):
    from waldo_amd import render as R
    wheel = torch.from_numpy(R.flow_wheel(128))
    h, w = 3, 129
    assert int(R.render_flow(torch.zeros(2, 2, h, w, device=dev)).max()) == 0             # a zero flow
    x = torch.randn(2, 2, h, w, generator=torch.Generator().manual_seed(3))
    bad = x.clone()
    bad[0, 0, :, ::2] = float("nan")   # NaN in u
    bad[1, 1, :, 1::2] = float("nan")  # NaN in v
    got = R.render_flow(bad.to(dev)).cpu()
    assert int(got[0, :, :, ::2].max()) == 0 and int(got[1, :, :, 1::2].max()) == 0
    assert torch.equal(got[0, :, :, 1::2], R.render_flow(x.to(dev)).cpu()[0, :, :, 1::2])
    # |flow| large, directions at the CENTRES of the bins (theta stable): r clamps to 1, the bytes are the wheel's
    k = torch.arange(h * w) % 128
    phi = (2 * (k.double() + 0.5) / 128 - 1) * np.pi
    big = torch.stack([3.0 * torch.cos(phi), 3.0 * torch.sin(phi)]).float().view(1, 2, h, w)
    for q, want in (("trunc", (wheel * 255.0).to(torch.uint8)), ("round", (wheel * 255.0 + 0.5).to(torch.uint8))):
        got = R.render_flow(big.to(dev), quantize=q, layout="nhwc").cpu().view(-1, 3)
        assert torch.equal(got, want[k]), q
    # a wheel of another size, read from global memory (more rows than the kernel keeps in LDS), and mul
    wheel2 = R.flow_wheel(640)
    k2 = torch.arange(h * w) % 640
    phi = (2 * (k2.double() + 0.5) / 640 - 1) * np.pi
    big = torch.stack([3.0 * torch.cos(phi), 3.0 * torch.sin(phi)]).float().view(1, 2, h, w)
    got = R.render_flow(big.to(dev), wheel=wheel2, layout="nhwc").cpu().view(-1, 3)
    assert torch.equal(got, (torch.from_numpy(wheel2) * 255.0).to(torch.uint8)[k2])
    assert int(R.render_flow(big.to(dev), mul=0.0).max()) == 0


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_flow_layouts_dtypes_and_strided_sources(dev, hw):
    from waldo_amd import render as R
    h, w = hw
    g = torch.Generator().manual_seed(11)
    flow = (torch.randn(2, 3, 4, 2, h, w, generator=g) * 0.08).to(dev)    # pred_flow's shape (B, Tc, Tp, 2, H, W)
    base = R.render_flow(flow)
    assert base.shape == (2, 3, 4, 3, h, w)
    assert torch.equal(R.render_flow(flow, layout="nhwc"), base.permute(0, 1, 2, 4, 5, 3))
    assert torch.equal(R.render_flow(flow[:, -1]), base[:, -1])            # the last context: a strided slice
    assert torch.equal(R.render_flow(flow[:, :, 1:3]), base[:, :, 1:3])    # leading dimensions that do not flatten
    assert torch.equal(R.render_flow(flow[0, 0, 0]), base[0, 0, 0])
    wide = torch.zeros(2, 2, h, w + 5, device=dev)
    wide[..., 2:2 + w] = flow[:, 0, 0]
    assert torch.equal(R.render_flow(wide[..., 2:2 + w]), base[:, 0, 0])   # rows not dense: element loads
    for dtype in (torch.bfloat16, torch.float16):                         # a 16-bit value is widened exactly
        low = flow.to(dtype)
        assert torch.equal(R.render_flow(low), R.render_flow(low.float())), dtype
        assert torch.equal(R.render_flow(low, quantize="round", layout="nhwc"),
                           R.render_flow(low.float(), quantize="round", layout="nhwc")), dtype
    assert not torch.equal(R.render_flow(flow, quantize="round"), base)


# ---------------------------------------------------------------------------------------------------------- round trips
def test_class_ids_invert_layout_to_logits_and_feed_pack_clip(dev):
    from waldo_amd import functional as WF
    from waldo_amd import render as R
    from waldo_amd.tools import io as wio
    nl, h, w = 20, 12, 37
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, nl, (2, 3, h, w), generator=g)
    lyt = torch.stack([torch.stack([wio.layout_to_logits(ids[b, t], nl) for t in range(3)]) for b in range(2)]).to(dev)
    got = R.class_ids(lyt)
    assert torch.equal(got.cpu(), ids.to(torch.uint8))
    rgb = (torch.rand(2, 3, 3, h, w, generator=g) * 2 - 1).to(dev)
    clip = WF.pack_clip(WF.frames_to_bytes(rgb), got, nl)
    assert torch.equal(clip.data[..., 3], got)
    assert torch.equal(clip.unpack()[:, :, 3:], lyt)
    assert torch.equal(R.class_ids(clip.unpack()[:, :, 3:]), got)


# ---------------------------------------------------------------------------------------------------------- predict
FRAMES, CTX = 6, 4
NEW_KEYS = ("rec_lyt_ids", "rec_sem_lyt", "pred_lyt_ids", "pred_sem_lyt", "pred_flow_rgb")


class _Job:
    """predict()'s arguments at the demo's smallest option set: dim 16, aspect 2, 3 objects, 6 frames, 4 contexts, two
    clips, as an fp32 clip and as a packed one."""

    def __init__(self, dev):
        from waldo_amd import functional as WF
        from waldo_amd.nets.lvd import Warper
        from waldo_amd.nets.wif import WIF
        from waldo_amd.tools import demo
        self.opt = demo.demo_opt(dim=16, aspect_ratio=2.0, num_obj=3)
        self.clips = 2
        g = torch.Generator().manual_seed(5)
        rgb = torch.randint(0, 256, (self.clips, FRAMES, 3, 16, 32), generator=g, dtype=torch.uint8)
        cls = torch.randint(0, 20, (self.clips, FRAMES, 4, 4), generator=g).repeat_interleave(4, 2).repeat_interleave(8, 3)
        self.packed = WF.pack_clip(rgb, cls, self.opt.num_lyt).to(dev)
        full = self.packed.unpack()
        self.vid, self.lyt = full[:, :, :3].contiguous(), full[:, :, 3:].contiguous()
        self.warper = Warper(self.opt).to(dev)
        self.wif = WIF(self.opt, unet=demo.UniformFusionUNet()).to(dev)
        self.net = demo.synthetic_network_outputs(self.opt, self.clips, FRAMES, CTX, seed=2, device=dev)

    def predict(self, form="fp32", **kw):
        from waldo_amd.tools import demo
        vid, lyt = (self.packed, None) if form == "packed" else (self.vid, self.lyt)
        return demo.predict(self.opt, self.warper, self.wif, vid, lyt, self.net, CTX, **kw)


@pytest.fixture(scope="module")
def job(dev):
    return _Job(dev)


def _decoded_layouts(job, monkeypatch, form):
    """A render=None call, and the fp32 layout channels its decodes produced (predict drops them): (result, rec, pred)."""
    from waldo_amd.tools import demo
    seen = []
    real = demo.decode_output

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append(res[0])
        return res

    monkeypatch.setattr(demo, "decode_output", spy)
    ref = job.predict(form)
    monkeypatch.setattr(demo, "decode_output", real)
    if len(seen) == 1:  # the merged decode: the reconstruction's units, then the prediction's
        return ref, seen[0][:, :FRAMES, 3:], seen[0][:, FRAMES:, 3:]
    return ref, seen[0][:, :, 3:], seen[1][:, :, 3:]


@pytest.mark.parametrize("form", ["fp32", "packed"])
@pytest.mark.parametrize("merge", [True, False], ids=["merged", "two_decodes"])
def test_predict_render(dev, job, monkeypatch, merge, form):
    from waldo_amd import render as R
    from waldo_amd.tools import demo
    monkeypatch.setattr(demo, "MERGE_DECODES", merge)
    ref, rec_lyt, pred_lyt = _decoded_layouts(job, monkeypatch, form)
    assert rec_lyt.shape[2] == 20 and pred_lyt.shape[1] == FRAMES - CTX
    got = job.predict(form, render="trunc")
    assert set(got) == set(ref) | set(NEW_KEYS)
    for key in ref:  # every old key bit-equal
        assert got[key].dtype == ref[key].dtype and torch.equal(got[key], ref[key]), key
    pal = R.layer_palette(20)
    for phase, lyt in (("rec", rec_lyt), ("pred", pred_lyt)):
        ids, sem = got[phase + "_lyt_ids"], got[phase + "_sem_lyt"]
        assert ids.dtype == sem.dtype == torch.uint8
        assert ids.shape == (2, lyt.shape[1], 16, 32) and sem.shape == (2, lyt.shape[1], 3, 16, 32)
        assert torch.equal(ids, R.class_ids(lyt)) and torch.equal(ids.cpu(), ref_ids(lyt)), phase
        assert torch.equal(sem, R.render_argmax(lyt, pal)), phase
        assert len(ids.unique()) > 3  # (a layout, not a constant)
    assert got["pred_flow_rgb"].shape == (2, CTX, FRAMES - CTX, 3, 16, 32)
    assert torch.equal(got["pred_flow_rgb"], R.render_flow(ref["pred_flow"]))
    rounded = job.predict(form, render="round", palette=list(range(60)))
    assert torch.equal(rounded["pred_flow_rgb"], R.render_flow(ref["pred_flow"], quantize="round"))
    assert torch.equal(rounded["rec_lyt_ids"], got["rec_lyt_ids"])
    assert torch.equal(rounded["pred_sem_lyt"], R.render_argmax(pred_lyt, R.semantic_palette(list(range(60)))))
    # the ids and the byte frames are what pack_clip takes
    by = job.predict(form, render="trunc", out_bytes="round")
    from waldo_amd import functional as WF
    clip = WF.pack_clip(by["rec_vid"], by["rec_lyt_ids"], 20)
    assert torch.equal(clip.data[..., 3], got["rec_lyt_ids"])


def test_predict_render_does_not_depend_on_the_decode_route(dev, job, monkeypatch):
    from waldo_amd.tools import demo
    merged = job.predict(render="trunc")
    monkeypatch.setattr(demo, "MERGE_DECODES", False)
    two = job.predict(render="trunc")
    for key in NEW_KEYS:
        assert torch.equal(merged[key], two[key]), key
    with pytest.raises(ValueError, match="render"):
        job.predict(render="floor")


@pytest.mark.parametrize("world", [2, 3])
def test_predict_sharded_carries_the_renders(dev, job, world):
    from waldo_amd.tools import demo
    one = job.predict(render="trunc")
    blocks = [demo.predict_sharded(job.opt, job.warper, job.wif, job.vid, job.lyt, job.net, CTX, r, world, render="trunc")
              for r in range(world)]
    for key in NEW_KEYS:
        full = torch.cat([blk[key] for blk in blocks], dim=0)
        assert full.dtype == torch.uint8, key
        got = demo.units_to_clips(key, full, job.clips, FRAMES, CTX, world, job.vid)
        assert got.shape == one[key].shape and torch.equal(got, one[key]), key


def test_predict_renders_the_context_layers_when_alpha_is_returned(dev, job):
    """With the inpainter's switch on, predict returns ``pred_alpha`` and the render of its layers."""
    from waldo_amd import render as R
    from waldo_amd.tools import demo
    import copy
    opt = copy.copy(job.opt)
    opt.use_inpainter = True
    res = demo.predict(opt, job.warper, job.wif, job.vid, job.lyt, job.net, CTX, render="trunc")
    assert "pred_alpha" in res and "ctx_obj_lyt" in res
    alpha = res["pred_alpha"]
    L = alpha.shape[-3]
    assert L == job.opt.num_obj + 1
    assert torch.equal(res["ctx_obj_lyt"], R.render_argmax(alpha, R.layer_palette(L)))
    assert res["ctx_obj_lyt"].shape == (*alpha.shape[:-3], 3, *alpha.shape[-2:])


# ---------------------------------------------------------------------------------------------------------- no host work
def test_no_synchronisation_and_graph_replay(dev):
    from waldo_amd import render as R
    from waldo_amd.graphs import GraphedCall
    c, h, w = 20, 12, 37
    x = class_frames(c, h, w, torch.float32).to(dev)[:, :, 3:3 + c].contiguous()
    flow = (torch.randn(2, 3, 2, h, w, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    pal = R.layer_palette(c)

    def fn(x, flow):
        rgb, ids = R.render_argmax(x, pal, layout="nhwc", return_ids=True)
        return R.class_ids(x), rgb, ids, R.render_flow(flow)

    eager = [t.clone() for t in fn(x, flow)]  # (the warm-up: the tables reach the device here)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = fn(x, flow)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(again, eager):
        assert torch.equal(a, b)
    with torch.no_grad():
        graphed = GraphedCall(fn, x, flow)
        for seed in (2, 3):
            x2 = class_frames(c, h, w, torch.float32, seed=seed).to(dev)[:, :, 3:3 + c].contiguous()
            flow2 = (torch.randn(2, 3, 2, h, w, generator=torch.Generator().manual_seed(seed)) * 0.1).to(dev)
            want = fn(x2, flow2)
            for a, b in zip(graphed(x2, flow2), want):
                assert torch.equal(a, b)


def test_demo_run_writes_the_renders(dev, tmp_path):
    """``demo --render --palette FILE``: the palette file is parsed, predict()'s renders come back from run() and the
    pictures are written as they are (the PNGs of the last frames hold the very bytes)."""
    from waldo_amd import render as R
    from waldo_amd.tools import demo
    from waldo_amd.tools import io as wio
    clip = os.path.join(ROOT, "tests", "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")
    ints = [(7 * i) % 256 for i in range(60)]
    path = tmp_path / "palette.txt"
    path.write_text(", ".join(str(v) for v in ints[:30]) + "\n" + " ".join(str(v) for v in ints[30:]) + "\n")
    palette = demo.read_palette_file(str(path))
    assert palette == ints
    out = tmp_path / "out"
    res = demo.run(clip, str(out), dim=32, device=str(dev), render="trunc", palette=palette)
    plain = demo.run(clip, None, dim=32, device=str(dev))
    assert set(res) == set(plain) | set(NEW_KEYS)
    assert torch.equal(res["pred_flow_rgb"], R.render_flow(plain["pred_flow"]))
    colours = {tuple(c) for c in res["rec_sem_lyt"][0].permute(0, 2, 3, 1).reshape(-1, 3).cpu().tolist()}
    assert colours <= {tuple(c) for c in R.semantic_palette(ints).tolist()} and len(colours) > 1
    for key, last in (("rec_sem_lyt", res["rec_sem_lyt"][0, -1]), ("pred_sem_lyt", res["pred_sem_lyt"][0, -1]),
                      ("pred_flow_rgb", res["pred_flow_rgb"][0, -1, -1])):
        assert os.path.getsize(out / (key + ".gif")) > 0, key
        assert torch.equal(wio.load_video_u8(str(out / (key + "_last.png")))[0], last.cpu()), key
    assert torch.equal(wio.load_video_u8(str(out / "rec_sem_lyt.gif")), res["rec_sem_lyt"][0].cpu())  # (<= 20 colours)
