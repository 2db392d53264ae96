"""GPU: the byte output (include/waldo_hip.h "Byte output"): functional.frames_to_bytes / wif_fuse_bytes, out_bytes of
WIF.forward and of tools.demo's predict / predict_sharded.  Every comparison is bit for bit.

The reference is the reference's own expression (tools/utils.py:246-264: normalize, * 255, .to(uint8); "round": + 0.5
before the cast, tools.io._to_uint8) written out below and evaluated on the device in fp32."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SPANS = [(-1.0, 1.0), (0.0, 1.0), (-0.3, 2.5)]
QUANTS = ["trunc", "round"]
LAYOUTS = ["nchw", "nhwc"]


def _f32(v):
    return ctypes.c_float(v).value


def ref_bytes(x, span=(-1.0, 1.0), quantize="trunc"):
    """((x.clamp(lo, hi) - lo) / (hi - lo) * 255 [+ 0.5]).to(uint8) in fp32, a 16-bit x widened first.  lo and hi - lo
    are DEVICE tensors: with a host scalar as the divisor the framework multiplies by its reciprocal instead of dividing."""
    lo, hi = _f32(span[0]), _f32(span[1])
    x = x.float()
    lo_t = torch.tensor(lo, dtype=torch.float32, device=x.device)
    rng_t = torch.tensor(hi, dtype=torch.float32, device=x.device) - lo_t
    u = (x.clamp(lo, hi) - lo_t) / rng_t
    y = u * 255.0
    if quantize == "round":
        y = y + 0.5
    return y.to(torch.uint8)


def expected_bytes(x, span, quantize):
    """ref_bytes on the finite values; 0 at a NaN; 0 / 255 at -inf / +inf (the header's NaN rule)."""
    xf = x.float()
    want = ref_bytes(torch.where(torch.isfinite(xf), xf, torch.zeros_like(xf)), span, quantize)
    want = torch.where(torch.isnan(xf), torch.zeros_like(want), want)
    want = torch.where(xf == float("inf"), torch.full_like(want, 255), want)
    return torch.where(xf == float("-inf"), torch.zeros_like(want), want)


def to_layout(nchw, layout):
    return nchw if layout == "nchw" else nchw.movedim(-3, -1).contiguous()


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_16_bit_value(dev, dtype):
    from waldo_amd import functional as WF
    bits = (torch.arange(65536, device=dev) - 32768).to(torch.int16)
    x = bits.view(dtype).view(1, 1, 256, 256)
    xf = x.float()
    assert int(torch.isnan(xf).sum()) > 0 and int(torch.isinf(xf).sum()) == 2
    for span in SPANS:
        for q in QUANTS:
            got = WF.frames_to_bytes(x, span=span, quantize=q)
            assert got.dtype == torch.uint8 and got.shape == x.shape
            want = expected_bytes(x, span, q)
            bad = (got != want).nonzero()
            assert bad.numel() == 0, (span, q, bad[:4].tolist(), xf[got != want][:4].tolist())
            assert int(got[torch.isnan(xf)].max()) == 0
            assert got[xf == float("inf")].tolist() == [255] and got[xf == float("-inf")].tolist() == [0]


def _threshold_values(span, dev):
    """The fp32 values nearest lo + k / 255 range and lo + (k - 0.5) / 255 range, k = 0 .. 255, with four ulp-neighbours
    on each side, and the special values."""
    lo, hi = _f32(span[0]), _f32(span[1])
    rng = _f32(hi - lo)
    k = torch.arange(256, dtype=torch.float64)
    centre = torch.cat([lo + k / 255.0 * rng, lo + (k - 0.5) / 255.0 * rng]).float()
    ints = centre.view(torch.int32).unsqueeze(1) + torch.arange(-4, 5, dtype=torch.int32).unsqueeze(0)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, 1e30, -1e30, float("inf"),
                            float("-inf"), float("nan"), lo, hi], dtype=torch.float32)
    return torch.cat([ints.flatten().view(torch.float32), special]).to(dev)


@pytest.mark.parametrize("span", SPANS)
def test_fp32_thresholds(dev, span):
    from waldo_amd import functional as WF
    v = _threshold_values(span, dev)
    x = v.view(1, 1, 1, -1)
    for q in QUANTS:
        got = WF.frames_to_bytes(x, span=span, quantize=q)
        want = expected_bytes(x, span, q)
        assert torch.equal(got, want), (span, q, v[(got != want).flatten()][:6].tolist())
    # the thresholds are where they should be: k / 255 reaches byte k under "round", at the latest one ulp above it
    # under "trunc" (the value nearest lo + k / 255 range may lie just below the exact threshold)
    lo, hi = _f32(span[0]), _f32(span[1])
    exact = (lo + torch.arange(256, dtype=torch.float64) / 255.0 * _f32(hi - lo)).float().to(dev).view(1, 1, 1, -1)
    assert torch.equal(WF.frames_to_bytes(exact, span=span, quantize="round").flatten().cpu(),
                       torch.arange(256, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------ shapes
SHAPES = [(2, 3, 3, 7), (1, 3, 5, 13), (3, 3, 2, 65), (1, 3, 1, 1), (2, 3, 4, 64),
          (1, 3, 40, 111)]  # (the last: a frame of several workgroups, 13 320 values in one row)


def _values(shape, dev, seed, dtype=torch.float32):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(shape, generator=g, device=dev) * 2.6 - 1.3).to(dtype)


def _guarded(shape, offset, dev, pad=0):
    """A uint8 view of `shape` (frames dense, `pad` bytes between frames) starting `offset` bytes into the 32-byte aligned
    part of a buffer filled with 0xA5, and the buffer."""
    n, frame = shape[0], shape[1] * shape[2] * shape[3]
    buf = torch.full((64 + n * (frame + pad) + 64,), 0xA5, dtype=torch.uint8, device=dev)
    body = buf[32 + offset:32 + offset + n * (frame + pad)].view(n, frame + pad)
    return body[:, :frame].view(shape), buf, body


def _assert_guard_intact(buf, body, out, offset):
    mask = torch.ones_like(buf, dtype=torch.bool)
    frame = out[0].numel()
    start = 32 + offset
    for i in range(out.shape[0]):
        mask[start + i * body.shape[1]:start + i * body.shape[1] + frame] = False
    assert bool((buf[mask] == 0xA5).all()), "bytes outside out were written"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shapes_that_break_vector_paths(dev, shape, layout, dtype):
    from waldo_amd import functional as WF
    n, c, h, w = shape
    q = "trunc"
    x = _values(shape, dev, 1, dtype)
    want = to_layout(ref_bytes(x), layout)
    got = WF.frames_to_bytes(x, layout=layout)
    assert got.shape == want.shape and torch.equal(got, want)
    # a 3-of-5-channel slice, read in place
    big = _values((n, 5, h, w), dev, 2, dtype)
    assert torch.equal(WF.frames_to_bytes(big[:, :3], layout=layout), to_layout(ref_bytes(big[:, :3]), layout))
    assert torch.equal(WF.frames_to_bytes(big[:, 1:4], layout=layout, quantize="round"),
                       to_layout(ref_bytes(big[:, 1:4], quantize="round"), layout))
    # a [:, 1:3] time slice of a 5-D clip (two clips: the leading dimensions do not flatten by stride; one clip: they do)
    for clips in (2, 1):
        clip = _values((clips, 4, c, h, w), dev, 3, dtype)
        got = WF.frames_to_bytes(clip[:, 1:3], layout=layout)
        assert got.shape[:2] == (clips, 2) and torch.equal(got, to_layout(ref_bytes(clip[:, 1:3]), layout))
    # rows that are not dense in the source (a crop along W) and planes that are not (a crop along H)
    wide = _values((n, c, h + 2, w + 3), dev, 4, dtype)
    for view in (wide[..., :w], wide[:, :, 1:h + 1, :w], wide[:, :, 1:h + 1]):
        assert torch.equal(WF.frames_to_bytes(view, layout=layout), to_layout(ref_bytes(view), layout))
    # a source that starts one element into its storage
    flat = _values((x.numel() + 1,), dev, 5, dtype)
    shifted = flat[1:].view(shape)
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(WF.frames_to_bytes(shifted, layout=layout), to_layout(ref_bytes(shifted), layout))
    # out= views that start one and three bytes into their storage, and frames with a gap between them; the bytes
    # around them stay as they were
    oshape = shape if layout == "nchw" else (n, h, w, c)
    for offset, pad in ((1, 0), (3, 0), (0, 0), (2, 5)):
        out, buf, body = _guarded(oshape, offset, dev, pad)
        assert out.data_ptr() % 4 == offset % 4
        res = WF.frames_to_bytes(x, layout=layout, quantize=q, out=out)
        assert res is out and torch.equal(out, want), (offset, pad)
        _assert_guard_intact(buf, body, out, offset)


def test_out_is_validated(dev):
    from waldo_amd import functional as WF
    x = _values((2, 3, 4, 8), dev, 0)
    with pytest.raises(ValueError):
        WF.frames_to_bytes(x, out=torch.empty(2, 3, 4, 8, device=dev))                       # not uint8
    with pytest.raises(ValueError):
        WF.frames_to_bytes(x, out=torch.empty(2, 4, 8, 3, dtype=torch.uint8, device=dev))    # the other layout's shape
    with pytest.raises(ValueError):
        WF.frames_to_bytes(x, out=torch.empty(2, 3, 4, 16, dtype=torch.uint8, device=dev)[..., ::2])  # frames not dense
    with pytest.raises(ValueError):
        WF.frames_to_bytes(_values((2, 4, 4, 8), dev, 0), layout="nhwc")                     # C != 3
    assert WF.frames_to_bytes(x[:0]).shape == (0, 3, 4, 8)
    y = x.clone().requires_grad_()
    assert not WF.frames_to_bytes(y).requires_grad


# ------------------------------------------------------------------------------------------ packed source
def _packed_every_byte(dev, b=2, t=3, h=8, w=37, seed=0):
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (b, t, h, w, 4), generator=g, dtype=torch.uint8)
    data[..., 3] %= 20
    ramp = torch.arange(256, dtype=torch.uint8)
    data[0, 0].view(-1, 4)[:256, 0] = ramp
    data[0, 1].view(-1, 4)[:256, 1] = ramp.flip(0)
    data[1, 2].view(-1, 4)[:256, 2] = ramp
    return WF.PackedClip(data.to(dev), 20)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_packed_source(dev, layout):
    from waldo_amd import functional as WF
    clip = _packed_every_byte(dev)
    rgb = clip.rgb()
    for q in QUANTS:
        got = WF.frames_to_bytes(clip, quantize=q, layout=layout)
        assert torch.equal(got, WF.frames_to_bytes(rgb, quantize=q, layout=layout)), q
        assert torch.equal(got, to_layout(ref_bytes(rgb, quantize=q), layout)), q
        for view in (clip[:, 1:3], clip[1:2, 1:3], clip[1:2]):  # (copied once; read in place; read in place)
            assert torch.equal(WF.frames_to_bytes(view, quantize=q, layout=layout),
                               to_layout(ref_bytes(view.rgb(), quantize=q), layout)), q
    # "round" gives the clip's bytes back, "trunc" does not
    own = clip.data[..., :3].movedim(-1, 2)
    assert torch.equal(WF.frames_to_bytes(clip, quantize="round"), own)
    assert not torch.equal(WF.frames_to_bytes(clip, quantize="trunc"), own)


def test_packed_table_differs_from_the_bytes_in_the_63_known_positions(dev):
    """The device table of a packed source against tests/test_bytes_abi.py's host expression."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.io import rgb_from_u8
    ramp = torch.arange(256, dtype=torch.uint8)
    data = torch.stack([ramp, ramp, ramp, torch.zeros_like(ramp)], dim=-1).view(1, 1, 1, 256, 4)
    got = WF.frames_to_bytes(WF.PackedClip(data.to(dev), 1), quantize="trunc").cpu()
    u = (rgb_from_u8(ramp).clamp(-1.0, 1.0) - -1.0) / 2.0
    host = (u * 255).to(torch.uint8)
    assert int((host != ramp).sum()) == 63
    for c in range(3):
        assert torch.equal(got[0, 0, c, 0], host)


# ------------------------------------------------------------------------------------------ the fused epilogue
def _wif_inputs(dev, tc, c, co, h, w, vd=torch.float32, nd=torch.float32, b=2, t=2, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    vid = (torch.randn(b, t, tc, c, h, w, generator=g, device=dev) * 1.2).to(vd)
    net = (torch.randn(b, t, tc, co, h, w, generator=g, device=dev) * 0.7).to(nd)
    return vid, net


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(7, 9), (8, 16), (3, 5), (40, 52)])  # (the last: several workgroups per frame)
def test_wif_fuse_bytes_equals_the_two_launches(dev, hw, layout):
    from waldo_amd import functional as WF
    for tc in (1, 2, 4):
        for c, co in ((5, 4), (40, 5)):
            if hw == (40, 52) and c == 40:
                continue
            vid, net = _wif_inputs(dev, tc, c, co, *hw, seed=tc)
            for ab in (True, False):
                for q in QUANTS:
                    got = WF.wif_fuse_bytes(vid, net, ab=ab, quantize=q, layout=layout)
                    fp32 = WF.wif_fuse(vid, net, ab=ab)
                    want = WF.frames_to_bytes(fp32, quantize=q, layout=layout)
                    assert got.dtype == torch.uint8 and got.shape == want.shape
                    assert torch.equal(got, want), (tc, c, co, ab, q)
                    assert torch.equal(want, to_layout(ref_bytes(fp32, quantize=q), layout))
    vid, net = _wif_inputs(dev, 2, 5, 4, *hw)
    got = WF.wif_fuse_bytes(vid, net, span=(-0.3, 2.5), quantize="round", layout=layout)
    assert torch.equal(got, WF.frames_to_bytes(WF.wif_fuse(vid, net), span=(-0.3, 2.5), quantize="round", layout=layout))


@pytest.mark.parametrize("hw", [(8, 16), (7, 9)])
@pytest.mark.parametrize("nd", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("vd", [torch.float32, torch.float16, torch.bfloat16])
def test_wif_fuse_bytes_dtype_pairs(dev, vd, nd, hw):
    from waldo_amd import functional as WF
    vid, net = _wif_inputs(dev, 4, 6, 4, *hw, vd=vd, nd=nd, seed=7)
    for layout in LAYOUTS:
        got = WF.wif_fuse_bytes(vid, net, layout=layout)
        assert torch.equal(got, WF.frames_to_bytes(WF.wif_fuse(vid, net), layout=layout)), layout


def test_wif_fuse_bytes_is_forward_only(dev):
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    vid, net = _wif_inputs(dev, 2, 5, 4, 4, 8)
    for a, b in ((vid.clone().requires_grad_(), net), (vid, net.clone().requires_grad_())):
        with pytest.raises(WaldoHipError):
            WF.wif_fuse_bytes(a, b)
        with torch.no_grad():
            assert not WF.wif_fuse_bytes(a, b).requires_grad


@pytest.mark.parametrize("score", [True, False])
def test_wif_forward_out_bytes(dev, score):
    from waldo_amd import functional as WF
    from waldo_amd.nets.wif import WIF
    from waldo_amd.tools import demo
    b, tc, t, c, h, w = 2, 3, 2, 6, 5, 9
    torch.manual_seed(0)
    unet = torch.nn.Conv2d(c if score else tc * c, 4 if score else 3, 1)
    wif = WIF(demo.demo_opt(dim=16, ii_score=score), unet=unet).to(dev)
    vid = _values((b, tc, t, c, h, w), dev, 11)
    with torch.no_grad():
        fp32 = wif(vid)
        for q in QUANTS:
            got = wif(vid, out_bytes=q)
            assert got.dtype == torch.uint8 and got.shape == (b, t, 3, h, w)
            assert torch.equal(got, WF.frames_to_bytes(fp32, quantize=q)), q
        assert torch.equal(wif(vid), fp32) and wif(vid).dtype == torch.float32  # the default is what it was


# ------------------------------------------------------------------------------------------ predict
BYTE_KEYS = {"rec_vid": 3, "inp_rec_vid": 3, "pred_vid": 3, "inp_pred_vid": 3, "rec_disocc": 1, "pred_disocc": 1}
FRAMES, CTX = 6, 4


class _Job:
    """predict()'s arguments at demo options, dim 16, aspect 2, 3 objects, 6 frames, 4 contexts, two clips; the fp32
    results are computed once per (clip form, raw_dtype) and kept."""

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
        # (an fp32 clip that is NOT on the byte lattice: "trunc" then has something to cut)
        self.vid = (full[:, :, :3] + 0.003 * torch.randn(full[:, :, :3].shape, generator=g).to(dev)).contiguous()
        self.lyt = full[:, :, 3:].contiguous()
        self.warper = Warper(self.opt).to(dev)
        self.wif = WIF(self.opt, unet=demo.UniformFusionUNet()).to(dev)
        self.net = demo.synthetic_network_outputs(self.opt, self.clips, FRAMES, CTX, seed=2, device=dev)
        self._fp32 = {}

    def args(self, form):
        return (self.packed, None) if form == "packed" else (self.vid, self.lyt)

    def predict(self, form, raw_dtype, out_bytes=None):
        from waldo_amd.tools import demo
        vid, lyt = self.args(form)
        return demo.predict(self.opt, self.warper, self.wif, vid, lyt, self.net, CTX, raw_dtype=raw_dtype,
                            out_bytes=out_bytes)

    def fp32(self, form, raw_dtype):
        key = (form, raw_dtype)
        if key not in self._fp32:
            self._fp32[key] = self.predict(form, raw_dtype)
        return self._fp32[key]


@pytest.fixture(scope="module")
def job(dev):
    return _Job(dev)


@pytest.mark.parametrize("q", QUANTS)
@pytest.mark.parametrize("raw_dtype", [None, torch.bfloat16])
@pytest.mark.parametrize("form", ["fp32", "packed"])
def test_predict_out_bytes(dev, job, form, raw_dtype, q):
    from waldo_amd import functional as WF
    ref = job.fp32(form, raw_dtype)
    got = job.predict(form, raw_dtype, out_bytes=q)
    assert set(got) == set(ref)
    for key, ch in BYTE_KEYS.items():
        assert got[key].dtype == torch.uint8 and got[key].shape == ref[key].shape and got[key].shape[2] == ch, key
        assert ref[key].dtype == torch.float32
        assert torch.equal(got[key], WF.frames_to_bytes(ref[key], quantize=q)), key
        assert torch.equal(got[key], ref_bytes(ref[key], quantize=q)), key
    assert got["pred_flow"].dtype == torch.float32 and torch.equal(got["pred_flow"], ref["pred_flow"])
    assert got["rec_vid"].float().std() > 10  # not a blank clip
    if form == "packed" and q == "trunc":  # the context frames are quantised, not copied
        own = job.packed.data[:, :CTX, :, :, :3].movedim(-1, 2)
        assert not torch.equal(got["pred_vid"][:, :CTX], own)


@pytest.mark.parametrize("world", [2, 3, 5])
def test_predict_sharded_out_bytes(dev, job, world):
    """The ranks' uint8 blocks (all ranks one after the other in this process), put together with units_to_clips, are the
    one-rank byte result; a rank without units (4 predicted frames over 5 ranks) holds empty uint8 blocks."""
    from waldo_amd.tools import demo
    q = "trunc"
    one = job.predict("fp32", None, out_bytes=q)
    blocks = [demo.predict_sharded(job.opt, job.warper, job.wif, job.vid, job.lyt, job.net, CTX, r, world, out_bytes=q)
              for r in range(world)]
    for key, want in one.items():
        for blk in blocks:
            assert blk[key].dtype == want.dtype, key
        full = torch.cat([blk[key] for blk in blocks], dim=0)
        got = demo.units_to_clips(key, full, job.clips, FRAMES, CTX, world, job.vid, out_bytes=q)
        assert got.dtype == want.dtype and got.shape == want.shape, key
        assert torch.equal(got, want), key


def test_scores_of_bytes_equal_scores_of_quantised_fp32(dev):
    from waldo_amd import functional as WF
    from waldo_amd import metrics as M
    pred, real = _values((1, 2, 3, 32, 64), dev, 21), _values((1, 2, 3, 32, 64), dev, 22)
    want = M.frame_metrics(pred, real, metrics=("psnr", "ssim"), quantize="trunc")
    got = M.frame_metrics(WF.frames_to_bytes(pred), WF.frames_to_bytes(real), metrics=("psnr", "ssim"))
    for name in ("psnr", "ssim"):
        assert torch.equal(got[name], want[name]), name


def test_evaluate_prediction_takes_byte_results(dev, job):
    from waldo_amd.tools import demo
    want = demo.evaluate_prediction(job.fp32("fp32", None), job.vid)
    got = demo.evaluate_prediction(job.predict("fp32", None, out_bytes="trunc"), job.vid)
    for key in want:
        for name in want[key]:
            assert torch.equal(got[key][name], want[key][name]), (key, name)


def test_graph_replay(dev):
    from waldo_amd import functional as WF
    from waldo_amd.graphs import GraphedCall
    x = _values((2, 3, 5, 13), dev, 31)
    vid, net = _wif_inputs(dev, 2, 5, 4, 7, 9, seed=32)

    def fn(x, vid, net):
        return WF.frames_to_bytes(x, layout="nhwc"), WF.wif_fuse_bytes(vid, net)

    with torch.no_grad():
        graphed = GraphedCall(fn, x, vid, net)
        for seed in (33, 34):
            x2 = _values((2, 3, 5, 13), dev, seed)
            vid2, net2 = _wif_inputs(dev, 2, 5, 4, 7, 9, seed=seed)
            eager = fn(x2, vid2, net2)
            for a, b in zip(graphed(x2, vid2, net2), eager):
                assert torch.equal(a, b)
