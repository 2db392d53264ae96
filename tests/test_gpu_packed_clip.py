"""GPU: the packed clip (functional.PackedClip: [R, G, B, class id] bytes per pixel) against its unpacked fp32 form.
Every packed kernel must give the bits its fp32 twin gives on ``unpack()``, and decode_output / demo.predict on a packed
clip the bits they give on the fp32 clip."""
import pytest
import torch

from test_packed_clip_abi import unpacked_reference

pytestmark = pytest.mark.gpu


def random_clip(dev, b, t, nlyt, hd, wd, seed, max_cls=None):
    """Random RGB bytes and class ids in [0, max_cls) (default: ids up to 2 Nl + 3, so that some are >= Nl)."""
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (b, t, 3, hd, wd), generator=g, dtype=torch.uint8)
    cls = torch.randint(0, max_cls or 2 * nlyt + 4, (b, t, hd, wd), generator=g)
    return WF.pack_clip(rgb, cls, nlyt).to(dev)


@pytest.mark.parametrize("shape", [(1, 2, 20, 8, 16), (2, 3, 5, 7, 9), (1, 2, 0, 6, 10), (1, 1, 32, 3, 13)])
def test_unpack_equals_the_restatement(dev, shape):
    """unpack() == the torch restatement, odd and unaligned widths, class ids >= Nl, no layout at all."""
    b, t, nlyt, hd, wd = shape
    clip = random_clip(dev, b, t, nlyt, hd, wd, seed=sum(shape))
    got = clip.unpack()
    assert got.dtype == torch.float32 and got.shape == clip.shape
    assert torch.equal(got.cpu(), unpacked_reference(clip))
    assert torch.equal(clip.rgb().cpu(), unpacked_reference(clip)[:, :, :3])


@pytest.mark.parametrize("with_dist", [False, True])
@pytest.mark.parametrize("want_bits", [False, True])
@pytest.mark.parametrize("shape", [(1, 4, 3, 20, 12, 8, 16, 4), (2, 3, 2, 7, 5, 5, 6, 2)])
def test_downscale_and_flow_ctx_alpha(dev, with_dist, want_bits, shape):
    """downscale_frames and flow_ctx_alpha on the packed clip == on unpack(), bit for bit."""
    from waldo_amd import functional as WF
    b, t, tw, nlyt, nl, h, w, s = shape
    hd, wd = h * s, w * s
    clip = random_clip(dev, b, t, nlyt, hd, wd, seed=nl + s, max_cls=nlyt + 2)
    full = clip.unpack()
    assert torch.equal(WF.downscale_frames(clip, tw, 3, s), WF.downscale_frames(full, tw, 3, s))
    g = torch.Generator(device=dev).manual_seed(7)
    alpha_lr = torch.rand(b * tw, nl, h, w, generator=g, device=dev)
    alpha_lr[:, 2:] *= (torch.rand(b * tw, nl - 2, h, w, generator=g, device=dev) > 0.6)  # (sparse layers)
    occ = torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5
    dist = torch.softmax(torch.randn(b, nl - 1, nlyt, generator=g, device=dev), dim=2) if with_dist else None
    with torch.no_grad():
        got = WF.flow_ctx_alpha(alpha_lr, clip, dist, occ, tw, 3, s, want_bits=want_bits)
        ref = WF.flow_ctx_alpha(alpha_lr, full, dist, occ, tw, 3, s, want_bits=want_bits)
    assert len(got) == len(ref)
    for x, y in zip(got, ref):
        assert (x is None and y is None) or torch.equal(x, y)


# (b, t, tc, tp, nlyt, nl, h, w, s, tw, ghost, flow_amp): Tc = 4 without self (the FULL LDS instance), Tc = 1 / 2 (LDS,
# FULL = false), Wd % 4 != 0 (the plain kernel) and an odd Wd, Tc = 6 (the plain kernel for up to 8 contexts), large
# flows (the boxes do not fit: the contexts gather)
SHAPES = [(1, 4, 4, 1, 20, 12, 8, 16, 4, 4, False, 0.1), (2, 3, 2, 2, 4, 8, 5, 4, 16, 2, True, 0.1),
          (1, 2, 1, 2, 20, 4, 4, 8, 4, 2, False, 0.1), (1, 4, 3, 3, 5, 17, 6, 9, 2, 4, False, 0.1),
          (1, 2, 2, 1, 2, 8, 9, 7, 1, 2, False, 0.1), (1, 7, 6, 2, 3, 8, 4, 8, 4, 7, False, 0.1),
          (1, 4, 4, 1, 20, 12, 8, 16, 4, 4, False, 0.6)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_frame_warp_fuse_raw(dev, dtype, include_self, shape):
    """frame_warp_fuse_raw on the packed clip == on unpack(): out and raw bit for bit, every raw dtype; an index
    outside the clip sets the same status words."""
    from waldo_amd import functional as WF
    from waldo_amd._lib import IndexStatus
    b, t, tc, tp, nlyt, nl, h, w, s, tw, ghost, amp = shape
    if include_self:
        tp = t
    hd, wd = h * s, w * s
    c = 3 + nlyt
    g = torch.Generator(device=dev).manual_seed(nl * 10 + tc)
    m = b * tc * tp
    flow_lr = amp * torch.randn(m, nl, 2, h, w, generator=g, device=dev)
    isobj = torch.rand(m, nl - 1, h, w, generator=g, device=dev) * 1.2 if ghost else None
    a01 = torch.rand(b * tw, nl, hd, wd, generator=g, device=dev)
    occ = torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5
    ctx_ts = torch.randint(0, tw, (b, tc, tp), generator=g, device=dev)
    pred_ts = torch.randint(0, t, (tp,), generator=g, device=dev)
    clip = random_clip(dev, b, t, nlyt, hd, wd, seed=m + nl)
    full = clip.unpack()
    bad = ctx_ts.clone()
    bad[0, 0, 0] = t + 2  # (reported, clamped)
    with torch.no_grad():
        res = []
        for inp in (full, clip):
            r = WF.flow_ctx_warp_into_raw(flow_lr, isobj, a01, ctx_ts, pred_ts, occ, tw, s, c, include_self,
                                          raw_dtype=dtype)
            st = IndexStatus()
            out, raw = WF.frame_warp_fuse_raw(inp, r[0].view(b, tc, tp, 2, hd, wd), r[4], bad, status=st)
            torch.cuda.synchronize()
            res.append((out, raw, st.words.clone()))
    (out32, raw32, st32), (outp, rawp, stp) = res
    assert rawp.dtype == dtype
    assert torch.equal(outp, out32)
    assert torch.equal(rawp.contiguous().view(torch.uint8), raw32.contiguous().view(torch.uint8))
    assert st32[0] == t and torch.equal(stp, st32)


def small_opt():
    """32 x 32 layers decoded to a 128 x 128 raster (x 4: the fused path's power-of-two scale), 4 layers."""
    from waldo_amd.tools import demo
    return demo.demo_opt(dim=32, aspect_ratio=1.0, num_obj=3, num_lyt=20, load_dim=128)


def _decode_args(dev, opt=None, frames=6, ctx_len=4, seed=0):
    """demo's decode of a random packed clip: (opt, warper, packed clip, decode_output's other arguments)."""
    from waldo_amd.nets import lvd
    from waldo_amd.nets.lvd import Warper
    from waldo_amd.nets.wif import WIF
    from waldo_amd.tools import demo
    opt = opt or small_opt()
    hd, wd = opt.load_dim, int(opt.load_dim * opt.aspect_ratio)
    clip = random_clip(dev, 1, frames, 20, hd, wd, seed=seed, max_cls=20)
    net = {k: v.to(dev) for k, v in demo.synthetic_network_outputs(opt, 1, frames, ctx_len, seed=seed).items()}
    warper, wif = Warper(opt).to(dev), WIF(opt, unet=demo.UniformFusionUNet()).to(dev)
    captured = {}
    orig = demo.decode_output

    def grab(*args, **kw):
        captured["args"], captured["kw"] = args, kw
        return orig(*args, **kw)

    demo.decode_output = grab
    try:
        with torch.no_grad():
            demo._decode_block(opt, warper, wif, clip.unpack(), net, ctx_len, 1, list(range(frames)),
                               list(range(ctx_len, frames)))
    finally:
        demo.decode_output = orig
    assert lvd.decode_output is orig
    return opt, warper, clip, list(captured["args"][2:9])


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("raw_dtype", [None, torch.bfloat16])
@pytest.mark.parametrize("restrict,products", [(True, False), (True, True), (False, False)])
def test_decode_output_packed_equals_unpacked(dev, monkeypatch, restrict, raw_dtype, products):
    """decode_output on the packed clip == on unpack(): all seven outputs, bit for bit; on this fused no-grad path
    PackedClip.unpack is never called (no fp32 copy of the clip is made)."""
    from waldo_amd import functional as WF
    from waldo_amd.nets.lvd import decode_output
    opt, warper, clip, rest = _decode_args(dev)
    grid, occ, obj_alpha, bg_alpha, cls, ctx_ts, pred_ts = rest
    full = clip.unpack()
    warper.return_alpha = True
    with torch.no_grad():
        cp_full = warper.context_products(full, grid, occ, obj_alpha, bg_alpha, cls, 4) if products else None
        ref = [x.clone() if torch.is_tensor(x) else x for x in
               decode_output(warper, full, grid, occ, obj_alpha, bg_alpha, cls, ctx_ts, pred_ts, restrict_to_ctx=restrict,
                             ctx_products=cp_full, raw_dtype=raw_dtype)]

        def refuse(self):
            raise AssertionError("PackedClip.unpack called on the fused no-grad path")

        monkeypatch.setattr(WF.PackedClip, "unpack", refuse)
        cp = warper.context_products(clip, grid, occ, obj_alpha, bg_alpha, cls, 4) if products else None
        got = decode_output(warper, clip, grid, occ, obj_alpha, bg_alpha, cls, ctx_ts, pred_ts, restrict_to_ctx=restrict,
                            ctx_products=cp, raw_dtype=raw_dtype)
    assert len(got) == 7
    for i, (x, y) in enumerate(zip(got, ref)):
        assert _same(x, y), i
    if raw_dtype is not None:
        assert got[5].dtype == raw_dtype


def test_decode_output_packed_at_c5_size(dev, monkeypatch):
    """One clip at the C5 raster (512 x 1024, 12 layers): packed == unpacked, bit for bit, without unpack()."""
    from waldo_amd import functional as WF
    from waldo_amd.nets.lvd import decode_output
    from waldo_amd.tools.pipeline import recipe_opt
    opt, warper, clip, rest = _decode_args(dev, recipe_opt("C5"), frames=6, seed=1)
    full = clip.unpack()
    with torch.no_grad():
        ref = [x.clone() if torch.is_tensor(x) else x for x in decode_output(warper, full, *rest)]
        monkeypatch.setattr(WF.PackedClip, "unpack", lambda self: (_ for _ in ()).throw(AssertionError("unpack")))
        got = decode_output(warper, clip, *rest)
    for i, (x, y) in enumerate(zip(got, ref)):
        assert _same(x, y), i


def test_decode_output_packed_under_autograd(dev):
    """With autograd the packed clip is unpacked once and today's path runs: the outputs are identical, and so is every
    leaf gradient -- up to the run-to-run spread of the fp32 backward itself where that accumulates with atomics (two
    fp32 runs are compared as the yardstick)."""
    from waldo_amd.nets.lvd import decode_output
    opt, warper, clip, rest = _decode_args(dev, frames=5)
    grid, occ, obj_alpha, bg_alpha, cls, ctx_ts, pred_ts = rest
    full = clip.unpack()
    outs, grads = [], []
    for inp in (full, full, clip):
        oa = obj_alpha.detach().clone().requires_grad_()
        oc = occ.detach().clone().requires_grad_()
        r = decode_output(warper, inp, grid, oc, oa, bg_alpha, cls, ctx_ts, pred_ts)
        loss = sum(x.float().square().mean() for x in (r[0], r[1], r[5]))
        loss.backward()
        outs.append([x.detach() if torch.is_tensor(x) else x for x in r])
        grads.append((oa.grad, oc.grad))
    for i, (x, y) in enumerate(zip(outs[0], outs[2])):
        assert _same(x, y), i
    for ref, again, got in zip(*grads):
        assert got is not None and got.shape == ref.shape
        if torch.equal(ref, again):
            assert torch.equal(got, ref)
        else:
            spread = (ref - again).abs().max()
            assert (got - ref).abs().max() <= 4 * spread


def test_demo_predict_packed_equals_fp32(dev):
    """demo.predict on the golden demo clip: packed (load_clip(packed=True)) and fp32 inputs give equal dicts."""
    import os

    from test_packed_clip_abi import CLIP
    from waldo_amd.nets.lvd import Warper
    from waldo_amd.nets.wif import WIF
    from waldo_amd.tools import demo
    from waldo_amd.tools import io as wio
    opt = demo.demo_opt(dim=32, aspect_ratio=2.0, num_obj=3, num_lyt=20, load_dim=128)
    size = (128, 256)
    assert os.path.isdir(CLIP)
    ref_clip = wio.load_clip(CLIP, size, 20, max_frames=6)
    pk_clip = wio.load_clip(CLIP, size, 20, max_frames=6, packed=True)
    vid, lyt = ref_clip["vid"].unsqueeze(0).to(dev), ref_clip["lyt"].unsqueeze(0).to(dev)
    warper, wif = Warper(opt).to(dev), WIF(opt, unet=demo.UniformFusionUNet()).to(dev)
    net = demo.synthetic_network_outputs(opt, 1, 6, 4, seed=0, device=dev)
    ref = demo.predict(opt, warper, wif, vid, lyt, net, 4)
    got = demo.predict(opt, warper, wif, pk_clip["vid"].to(dev), None, net, 4)
    assert set(got) == set(ref)
    for k in ref:
        assert _same(got[k], ref[k]), k
