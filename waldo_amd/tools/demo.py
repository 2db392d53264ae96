"""BASELINE config C1 plumbing: WIF inference on a demo clip, reproducing the call order of the
reference's ``Synthesizer.predict`` (models/synthesizer.py:425-480) around the hot path.

    python -m waldo_amd.tools.demo --clip <dir of frame PNGs> --out <dir> [--dim 128 --num-obj 3]

What is real: the frames and layout maps of the clip (``waldo_amd.tools.io.load_clip``), every
warp / composite / fusion step (the HIP kernels behind ``nets.lvd`` / ``nets.flp`` / ``nets.wif``),
the tensor plumbing between them (``ctx_ts`` / ``pred_ts`` construction, the ``last_n_ctx``
window, the disocclusion bookkeeping, the future-prediction branch).  What is synthetic: the
outputs of the networks that are outside this path (layer / pose estimators,
object decoder conv stack, pose generator, UNet) -- seeded stand-ins with the right shapes:
smooth object blobs for the decoder's raw image, small smooth motions for the pose heads, and a
UNet stand-in that predicts a zero residual and uniform scores.  The same stand-ins feed the CPU
restatement of the chain in tests/test_demo.py, so it is checked end to end, not just exercised.
"""
import argparse
import os
import types

import torch
import torch.nn as nn

from .. import functional as WF
from .. import render as WR
from ..nets import flp
from ..nets.lvd import Warper, decode_output, decoder_tail, estimate_alpha_grid_occ
from ..nets.wif import WIF
from . import io as wio
from .utils import get_grid


def demo_opt(dim=128, aspect_ratio=1.0, num_obj=3, num_lyt=20, **over):
    """The option fields the path reads (Warper: models/nets/lvd.py:472-499; WIF: ii_score, ii_ab, and what
    ``WIF.with_unet`` builds the network from: the ii_* fields at the reference's defaults, tools/options.py:235,
    309-316, 392), at the C1 size: 128 x 128, 4 layers (3 objects + background)."""
    d = dict(latent_shape=[4, 4], obj_shape=[2, 2], time_dropout=0.0, num_obj=num_obj, patch_size=8,
             scale_factor=2, dim=dim, aspect_ratio=aspect_ratio, load_dim=0, num_perm_grid=1,
             normalize_alpha=False, use_lyt_filtering=True, use_lyt_opacity=False, weight_cls=True,
             min_cls=0.05, include_self=False, no_filter=False, allow_ghost=False, num_lyt=num_lyt,
             ii_score=True, ii_ab=True, last_n_ctx=0, no_future=False, pad_obj_alpha=2, use_inpainter=False,
             ii_embed_dim=512, ii_depth=4, ii_upmode="bilinear", ii_ft_hd=False, norm_layer_patch="ln2d",
             use_disocc=False, ctx_len=4)
    d.update(over)
    return types.SimpleNamespace(**d)


class UniformFusionUNet(nn.Module):
    """UNet stand-in: zero colour residual (channels 0-2), equal scores (channel 3) -- the fusion of
    wif.py:49-54 then averages the warped context frames with their sigmoid(alpha + 5) weights.  The zeros are
    made once per shape and handed out again (nobody writes to them): the stand-in for a network OUTSIDE the path
    should not put half a millisecond of fills into the pipeline's timing."""

    def __init__(self):
        super().__init__()
        self._zeros = {}

    def forward(self, x):
        key = (x.shape[0], tuple(x.shape[-2:]), x.device, x.dtype)
        z = self._zeros.get(key)
        if z is None:
            z = self._zeros[key] = x.new_zeros(x.shape[0], 4, *x.shape[-2:])
        return z


# Background motion of the stand-ins, as (drift of the 2 x 2 affine part, of the translation, of the per-point
# deltas) per frame step, in the pose heads' units.
#   "wild"        every one of the 6 + 2 Lb background pose values drifts independently (0.02 randn per frame):
#                 with Lb = 128 lattice points 1/8 of the frame apart, neighbouring control points end up a whole
#                 lattice cell apart after ten frames -- a folded warp (local stretch |d ix / dx| of the composited
#                 flow at 512 x 1024: median 1, 90 % quantile 7, 99 % quantile 30).  The stress case; rounds 1-3
#                 benchmarked the C4 / C5 pipelines on it.
#   "calibrated"  the same amplitudes for the rigid part and a tenth of them for the per-point deltas: the local
#                 stretch of the warp stays within what optical flow of real driving footage shows (RAFT flows of
#                 the reference's demo clips, datasets/demo_cityscapes/*_raft_128: |d ix / dx| 10 % / 99 % quantiles
#                 0.92 / 1.04 per frame step, mean |flow| 2.4 px of 256 and max 16 px per step; measured with
#                 tools_dev/flo_stats.py), accumulated over the 4 .. 13 frame steps a clip spans.
BG_MOTION = {"wild": (0.02, 0.02, 0.02), "calibrated": (0.01, 0.02, 0.002)}


def synthetic_network_outputs(opt, b, t, ctx_len, seed=0, device="cpu", motion="wild"):
    """Seeded stand-ins for what the networks outside the path would hand over, on ``device``."""
    g = torch.Generator().manual_seed(seed)
    no, nl = opt.num_obj, opt.num_lyt
    lo = opt.obj_shape[0] * opt.obj_shape[1]
    lb = opt.latent_shape[0] * opt.latent_shape[1]
    ho, wo = opt.obj_shape[0] * opt.patch_size, opt.obj_shape[1] * opt.patch_size
    # object decoder raw image: one soft blob per object (positive inside -> alpha ~ +1 after tanh)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, ho), torch.linspace(-1, 1, wo), indexing="ij")
    rad = 0.5 + 0.3 * torch.rand(b * no, 1, 1, 1, generator=g)
    raw = 4.0 * (rad - (xx ** 2 + yy ** 2).sqrt().view(1, 1, ho, wo) / 1.0)
    # pose heads (after tanh): per-object placement + a slow drift over time, small point deltas
    base = 0.6 * (torch.rand(b, 1, no, 6 + 2 * lo, generator=g) * 2 - 1)
    drift = 0.05 * torch.randn(b, 1, no, 6 + 2 * lo, generator=g) * torch.arange(t).view(1, t, 1, 1)
    obj = base + drift
    obj[..., 6:] = 0.1 * obj[..., 6:]
    obj[..., [0, 3]] = -0.2 + 0.2 * obj[..., [0, 3]]  # scales around bias_obj - 0.2
    obj[..., [1, 2]] = 0.2 * obj[..., [1, 2]]        # small shear
    bg = 0.02 * torch.randn(b, 1, 1, 6 + 2 * lb, generator=g) * torch.arange(t).view(1, t, 1, 1)
    lin, shift, pts = BG_MOTION[motion]  # ("wild" multiplies by 1: the same numbers as ever)
    bg[..., [0, 1, 2, 3]] *= lin / 0.02
    bg[..., [4, 5]] *= shift / 0.02
    bg[..., 6:] *= pts / 0.02
    occ_score = torch.randn(b, t, no, generator=g)
    cls = torch.softmax(2.0 * torch.randn(b, no, nl, generator=g), dim=-1)
    out = dict(raw=raw, pred_obj_pose=obj.reshape(b * t, no, -1), pred_bg_pose=bg.reshape(b * t, 1, -1),
               occ_score=occ_score, cls=cls)
    return {k: v.to(device) for k, v in out.items()}


_CONSTANTS = {}


def _cached(kind, opt, device, make):
    """The path's constant tensors (the pose heads' buffers, the padding mask, the background alpha) live on the
    device ONCE per option set, as a model's registered buffers do: made inside predict() they were ten small
    host-to-device copies per call -- each one a point where the host stops queueing kernels -- and kept the call
    from being captured into a HIP graph."""
    key = (kind, str(device), tuple(opt.obj_shape), tuple(opt.latent_shape), opt.patch_size, opt.scale_factor,
           opt.pad_obj_alpha, opt.dim, float(opt.aspect_ratio))
    if key not in _CONSTANTS:
        _CONSTANTS[key] = make()
    return _CONSTANTS[key]


def pose_buffers(opt, device):
    """Buffers of the pose heads (models/nets/flp.py:119-123) at the demo's option values."""
    return _cached("pose", opt, device, lambda: _pose_buffers(opt, device))


def _pose_buffers(opt, device):
    lo = opt.obj_shape[0] * opt.obj_shape[1]
    lb = opt.latent_shape[0] * opt.latent_shape[1]
    return dict(
        tgt_pts_obj=get_grid(*opt.obj_shape).view(1, 1, lo, 2).to(device),
        tgt_pts_bg=get_grid(*opt.latent_shape).view(1, 1, lb, 2).to(device),
        bias_obj=torch.tensor([[[0.5, 0.0, 0.0, opt.aspect_ratio * 0.5, 0.0, 0.0]]], device=device),
        mul_obj=torch.tensor([[[0.5, 0.5, 0.5, 0.5, 1.0, 1.0]]], device=device),
        bias_bg=torch.tensor([[[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]], device=device))


def obj_alpha_mask(opt, device):
    """lvd.py:27-34: zero border of ``pad_obj_alpha`` decoder pixels around the object canvas."""
    return _cached("mask", opt, device, lambda: _obj_alpha_mask(opt, device))


def _obj_alpha_mask(opt, device):
    ho = opt.obj_shape[0] * opt.patch_size * opt.scale_factor
    wo = opt.obj_shape[1] * opt.patch_size * opt.scale_factor
    po = opt.pad_obj_alpha * opt.scale_factor
    m = torch.ones(ho, wo, device=device)
    if po > 0:
        m[:po] = 0
        m[:, :po] = 0
        m[-po:] = 0
        m[:, -po:] = 0
    return m.view(1, 1, 1, ho, wo)


def _cached_by(key, make):
    if key not in _CONSTANTS:
        _CONSTANTS[key] = make()
    return _CONSTANTS[key]


def _cached_index(values, device):
    """A small index tensor on the device, made once (a fresh host-to-device copy per call would stall the
    launch queue: see _cached)."""
    key = ("index", str(device), tuple(values))
    if key not in _CONSTANTS:
        _CONSTANTS[key] = torch.tensor(list(values), device=device, dtype=torch.int64)
    return _CONSTANTS[key]


def _block_net(opt, net, b, t, b0, b1, sel, device):
    """The stand-ins' outputs for clips b0:b1 at the frames ``sel`` (ascending) of the clip's T."""
    if (b0, b1) == (0, b) and list(sel) == list(range(t)):
        return net
    no = opt.num_obj
    idx = _cached_index(sel, device)

    def frames(x):  # (B * T, ...) -> (nb * T', ...)
        x = x.view(b, t, *x.shape[1:])[b0:b1]
        return x.index_select(1, idx).reshape(-1, *x.shape[2:])

    return dict(raw=net["raw"][b0 * no:b1 * no], pred_obj_pose=frames(net["pred_obj_pose"]),
                pred_bg_pose=frames(net["pred_bg_pose"]), occ_score=net["occ_score"][b0:b1].index_select(1, idx),
                cls=net["cls"][b0:b1])


class SharedContext:
    """What the decodes of one step compute from a clip's CONTEXT alone -- the object alphas (decoder tail + padding
    mask), the context frames' control points, grids, inverted grids and occlusion matrices, and the composited
    full-resolution context alphas (``Warper.context_products``) -- kept from the first decode for the next one.
    ``Synthesizer.predict`` runs them once per decode (synthesizer.py:434-445 and 470-472); its second decode receives
    the context poses "as they came in" (flp.py:275-290), so the products are the same tensors' functions: reused when
    the stand-ins' outputs and the input frames are the SAME tensor objects, unmodified (identity + version counter),
    computed afresh otherwise.  Every value depends on its own (b, t) frame, so a decode that reuses them has the bits
    of one that does not (tests/test_gpu_pipeline.py)."""

    def __init__(self):
        self.key, self.value, self.held = None, None, ()

    @staticmethod
    def _key(tensors):
        return tuple((id(x), None if x.is_inference() else x._version) for x in tensors)

    def get(self, tensors, make):
        key = self._key(tensors)
        if self.key != key or any(a is not b for a, b in zip(self.held, tensors)):
            self.value, self.key, self.held = make(), key, tuple(tensors)  # (held: ids are not recycled meanwhile)
        return self.value


def _points_grids_occ(opt, warper, net, nb, nt):
    """Pose heads' affine (flp.py:259-273), Warper.forward and compute_occ for the ``nt`` frames of ``net``."""
    from ..nets.lvd import compute_occ
    no = opt.num_obj
    lo = opt.obj_shape[0] * opt.obj_shape[1]
    lb = opt.latent_shape[0] * opt.latent_shape[1]
    buf = pose_buffers(opt, net["pred_obj_pose"].device)
    obj_pose = flp.obj_pose_to_points(net["pred_obj_pose"], buf["tgt_pts_obj"], buf["mul_obj"], buf["bias_obj"])
    bg_pose = flp.bg_pose_to_points(net["pred_bg_pose"], buf["tgt_pts_bg"], buf["bias_bg"])
    grid = warper(obj_pose.view(nb, nt, no, lo, 2), bg_pose.view(nb, nt, 1, lb, 2))
    return grid, compute_occ(net["occ_score"])


def _decode_block(opt, warper, wif, real_input, net, ctx_len, nb, sel, where, shared=None, shared_key=None,
                  out_alpha=None, raw_dtype=None, out_bytes=None, palette=None, out_render=None):
    """One decode of predict() (estimate_alpha_grid_occ -> decode_output -> disocclusion test -> WIF fusion,
    synthesizer.py:434-460 / 464-484) for ``nb`` clips on the compact time axis ``sel`` (frame numbers: the context
    frames 0 .. ctx_len - 1, then the other frames whose poses the decode needs -- a frame may stand there twice, with
    the reconstruction's and with the prediction's poses), producing the units at the positions ``where`` of that axis.
    ``net`` holds the stand-ins' outputs for exactly those clips and axis entries (_block_net); ``real_input``
    (nb, >= ctx_len, C, Hd, Wd) at least the context frames.  ``shared`` (a ``SharedContext``): what depends on the
    context alone is taken from / left for the other decodes of the step (``shared_key``: the tensors whose identity
    vouches for it, when ``net`` is a per-block copy of them).  Returns (output (nb, n, 3, Hd, Wd), disocc
    (nb, n, 1, Hd, Wd), inpainted (nb, n, 3, Hd, Wd), flow (nb, Tc, n, 2, Hd, Wd)).  Every kernel of the chain works
    per (b, t) unit (the layout filter's class distribution per clip, over its context frames), so the bits of a frame
    do not depend on which other frames or clips are decoded beside it (tests/test_gpu_pipeline.py).  ``raw_dtype``:
    decode_output's (None = fp32; bf16 / fp16: the WIF input in 16 bits, fused by the 16-bit wif_fuse).  ``out_bytes``
    ("trunc" / "round"): output, disocc and inpainted come back as uint8 (``WF.frames_to_bytes``; the inpainted frames
    quantised inside the fusion kernel) -- the bytes the reference's save_vid writes of them; flow stays fp32.
    ``out_render`` (a list): receives ``(ids, rgb)``, the class ids (nb, n, Hd, Wd) of the decoded layout channels
    ``output[:, :, 3:]`` (read in place) and the same ids through ``palette`` (nb, n, 3, Hd, Wd), uint8, from one launch
    (``render.render_argmax``)."""
    no = opt.num_obj
    dev = real_input.device
    nt, n = len(sel), len(where)
    assert list(sel[:ctx_len]) == list(range(ctx_len)), "the compact time axis starts with the context frames"
    # `alpha` (2 a' - 1 on the context frames) is dropped by the reconstruction (synthesizer.py:445) and handed by the
    # prediction to net_ii.inpaint (synthesizer.py:472, 484), which reads it only with the inpainter on (wif.py:103):
    # without one the flow pass does not write it (as large as the a' it keeps)
    want_alpha = bool(getattr(opt, "use_inpainter", False))
    mask = obj_alpha_mask(opt, dev)
    bg_alpha = _cached("bg_alpha", opt, dev, lambda: torch.ones(1, 1, opt.dim, int(opt.dim * opt.aspect_ratio), device=dev))

    def frames_of(x, lo, hi):  # (nb * nt, ...) -> (nb * (hi - lo), ...)
        return x.view(nb, nt, *x.shape[1:])[:, lo:hi].reshape(-1, *x.shape[1:])

    def context_part():
        # decoder tail (lvd.py:245-254) + the alpha arithmetic of estimate_alpha_grid_occ (lvd.py:128-132); the context
        # frames' part of its Warper.forward and compute_occ (lvd.py:133-134); what decode_output computes from them
        obj_alpha = decoder_tail(net["raw"], init_bias=0.0, scale_factor=opt.scale_factor)
        obj_alpha = obj_alpha.view(nb, no, 1, *obj_alpha.shape[-2:])
        ctx_net = dict(pred_obj_pose=frames_of(net["pred_obj_pose"], 0, ctx_len),
                       pred_bg_pose=frames_of(net["pred_bg_pose"], 0, ctx_len), occ_score=net["occ_score"][:, :ctx_len])
        # (estimate_alpha_grid_occ with the context frames' poses: occ, masked object alphas, expanded bg alpha, grids)
        lo = opt.obj_shape[0] * opt.obj_shape[1]
        lb = opt.latent_shape[0] * opt.latent_shape[1]
        buf = pose_buffers(opt, dev)
        obj_pose = flp.obj_pose_to_points(ctx_net["pred_obj_pose"], buf["tgt_pts_obj"], buf["mul_obj"], buf["bias_obj"])
        bg_pose = flp.bg_pose_to_points(ctx_net["pred_bg_pose"], buf["tgt_pts_bg"], buf["bias_bg"])
        occ, obj_alpha, bga, grid = estimate_alpha_grid_occ(warper, obj_alpha, bg_alpha, obj_pose.view(nb, ctx_len, no, lo, 2),
                                                            bg_pose.view(nb, ctx_len, 1, lb, 2), ctx_net["occ_score"],
                                                            obj_alpha_mask=mask)
        prev = warper.return_alpha
        warper.return_alpha = want_alpha
        try:
            products = warper.context_products(real_input, grid, occ, obj_alpha, bga, net["cls"], ctx_len)
        finally:
            warper.return_alpha = prev
        return occ, obj_alpha, bga, grid, products

    if shared is not None:
        key = shared_key if shared_key is not None else (net["raw"], net["pred_obj_pose"], net["pred_bg_pose"],
                                                          net["occ_score"], net["cls"], real_input)
        occ_c, obj_alpha, bga, grid_c, products = shared.get(key, context_part)
        if nt > ctx_len:  # the frames beyond the context: their control points, grids and occlusion matrices
            new_net = dict(pred_obj_pose=frames_of(net["pred_obj_pose"], ctx_len, nt),
                           pred_bg_pose=frames_of(net["pred_bg_pose"], ctx_len, nt), occ_score=net["occ_score"][:, ctx_len:])
            grid_n, occ_n = _points_grids_occ(opt, warper, new_net, nb, nt - ctx_len)
            grid = [torch.cat([a, b], dim=1) for a, b in zip(grid_c, grid_n)]
            occ = torch.cat([occ_c, occ_n], dim=1)
        else:
            grid, occ = list(grid_c), occ_c
    else:
        # nothing to share with another decode: the whole axis in ONE call each of the pose heads' affine, Warper.forward
        # and compute_occ (estimate_alpha_grid_occ, lvd.py:126-135) -- no second set of launches for the context's grids,
        # nothing to concatenate; the context's products from the first ctx_len frames of those grids
        lo = opt.obj_shape[0] * opt.obj_shape[1]
        lb = opt.latent_shape[0] * opt.latent_shape[1]
        buf = pose_buffers(opt, dev)
        obj_alpha = decoder_tail(net["raw"], init_bias=0.0, scale_factor=opt.scale_factor)
        obj_alpha = obj_alpha.view(nb, no, 1, *obj_alpha.shape[-2:])
        obj_pose = flp.obj_pose_to_points(net["pred_obj_pose"], buf["tgt_pts_obj"], buf["mul_obj"], buf["bias_obj"])
        bg_pose = flp.bg_pose_to_points(net["pred_bg_pose"], buf["tgt_pts_bg"], buf["bias_bg"])
        occ, obj_alpha, bga, grid = estimate_alpha_grid_occ(warper, obj_alpha, bg_alpha, obj_pose.view(nb, nt, no, lo, 2),
                                                            bg_pose.view(nb, nt, 1, lb, 2), net["occ_score"],
                                                            obj_alpha_mask=mask)
        prev = warper.return_alpha
        warper.return_alpha = want_alpha
        try:
            products = warper.context_products(real_input, grid, occ, obj_alpha, bga, net["cls"], ctx_len)
        finally:
            warper.return_alpha = prev
    def make_ctx_ts():  # synthesizer.py:438-442
        ts = torch.arange(ctx_len, device=dev, dtype=torch.int64).view(1, -1, 1).expand(nb, -1, n)
        return WF.normalise_time_index(ts[:, -opt.last_n_ctx:] if opt.last_n_ctx > 0 else ts)

    # the frame indices of a decode, made ONCE per shape and kept (int64, contiguous: as the kernels take them): built
    # afresh per call (synthesizer.py:438-444 does) each would be a small host-to-device copy in the launch queue
    ctx_ts = _cached_by(("ctx_ts", str(dev), ctx_len, nb, n, opt.last_n_ctx), make_ctx_ts)
    pred_ts = _cached_index(where, dev)
    # decode_output + max_l alpha_ctx, which the fused flow pass produces as a by-product (the warper's switch and its
    # result are restored / cleared afterwards: no state is left on the module)
    prev, prev_alpha = warper.keep_alpha_ctx_max, warper.return_alpha
    warper.keep_alpha_ctx_max = True
    warper.return_alpha = want_alpha
    try:
        output, flow, _, alpha, _, raw_output, alpha_ctx = decode_output(warper, real_input, grid, occ, obj_alpha, bga,
                                                                         net["cls"], ctx_ts, pred_ts, ctx_products=products,
                                                                         raw_dtype=raw_dtype)
        mx = warper.alpha_ctx_max
    finally:
        warper.keep_alpha_ctx_max, warper.return_alpha = prev, prev_alpha
        warper.alpha_ctx_max = None
    # synthesizer.py:447-450: max / min over the contexts of max_l alpha_ctx, dmax[dmax - dmin > 1] = 0 -- one pass
    # over the flow pass's by-product (torch: aminmax, subtract, compare, masked_fill)
    if mx is None:  # == alpha_ctx.max(dim=3)[0] (NaN-propagating, as torch's), without the fused pass's by-product
        mx = alpha_ctx.amax(dim=3)
    dmax = WF.disocc_test(mx)
    if out_alpha is not None:
        out_alpha.append(alpha)
    if out_render is not None:
        rgb, ids = WR.render_argmax(output[:, :, 3:], palette, return_ids=True)
        out_render.append((ids, rgb))
    if out_bytes is not None:  # (the 3-channel slice and the map are read in place)
        return (WF.frames_to_bytes(output[:, :, :3], quantize=out_bytes),
                WF.frames_to_bytes(dmax.unsqueeze(2), quantize=out_bytes), wif(raw_output, out_bytes=out_bytes), flow)
    return output[:, :, :3], dmax.unsqueeze(2), wif(raw_output), flow  # (wif: synthesizer.py:460)


def _check_out_bytes(fn, out_bytes):
    if out_bytes is not None and out_bytes not in WF.BYTE_QUANTIZE:
        raise ValueError(f"{fn}: out_bytes must be None or one of {tuple(WF.BYTE_QUANTIZE)}, got {out_bytes!r}")


def _check_render(fn, render):
    if render is not None and render not in WR.QUANTIZE:
        raise ValueError(f"{fn}: render must be None or one of {tuple(WR.QUANTIZE)}, got {render!r}")


def _render_palette(palette, num_lyt):
    """The palette of the ``*_sem_lyt`` renders: the caller's (at least ``num_lyt`` rows of 3 bytes; a flat list of
    3 * Nl integers is a dataset palette as the reference's option holds it) or ``layer_palette(num_lyt)``."""
    if palette is None:
        return WR.layer_palette(num_lyt)
    if not torch.is_tensor(palette) and getattr(palette, "ndim", 1) == 1:
        palette = WR.semantic_palette(list(palette))
    if palette.shape[0] < num_lyt:
        raise ValueError(f"palette: {palette.shape[0]} rows for {num_lyt} layout classes")
    return palette


RENDER_KEYS = {"rec": ("rec_lyt_ids", "rec_sem_lyt"), "pred": ("pred_lyt_ids", "pred_sem_lyt", "pred_flow_rgb")}


@torch.no_grad()
def predict(opt, warper, wif, real_vid, real_lyt, net, ctx_len, raw_dtype=None, out_bytes=None, render=None,
            palette=None):
    """The hot-path part of Synthesizer.predict (models/synthesizer.py:434-480).  real_vid
    (B, T, 3, H, W), real_lyt (B, T, Nl, H, W); ``net`` = synthetic_network_outputs(...).  Or real_vid a
    ``WF.PackedClip`` of frames and class ids (``tools.io.load_clip(..., packed=True)``) and real_lyt None: the same
    results bit for bit, without an fp32 copy of the clip on the fused path.
    ``raw_dtype``: the element type of the WIF input ``raw_output`` (None = fp32; torch.bfloat16 / torch.float16 for a
    UNet under autocast -- decode_output).  Returns a dict of the tensors predict produces.
    ``out_bytes`` (None, "trunc" or "round"): the ``*_vid`` keys come back as uint8 with 3 channels and the two
    ``*_disocc`` keys as uint8 with 1 channel -- ``WF.frames_to_bytes`` of what they are without it ("trunc": the bytes
    the reference's save_vid -> dump_video writes of them, synthesizer.py:403-411), quantised on the device; ``pred_flow``
    and ``pred_alpha`` stay as they are.  The context frames in front of ``pred_vid`` / ``inp_pred_vid`` are quantised
    from the clip (a packed clip's bytes are not copied: "trunc" does not give them back).
    ``render`` (None, "trunc" or "round"): the decomposition as pictures, rendered on the device (``waldo_amd.render``;
    the reference's log_lyt / log_flow, synthesizer.py:396-401) -- every other key stays what it is without it, and these
    are added, all uint8: ``rec_lyt_ids`` / ``pred_lyt_ids`` (B, T', Hd, Wd), the argmax of the decoded layout channels
    ``output[:, :, 3:3 + Nl]`` (with the ``*_vid`` bytes the two tensors ``WF.pack_clip`` takes); ``rec_sem_lyt`` /
    ``pred_sem_lyt`` (B, T', 3, Hd, Wd), those ids through ``palette`` (``_render_palette``; default
    ``render.layer_palette(Nl)``) from the same launch; ``pred_flow_rgb`` (B, Tc, Tp, 3, Hd, Wd), ``render.render_flow`` of
    ``pred_flow`` -- the only one the quantisation mode ``render`` applies to; and, where ``pred_alpha`` is returned,
    ``ctx_obj_lyt``: its argmax over the layers through ``render.layer_palette(L)``."""
    _check_out_bytes("predict", out_bytes)
    _check_render("predict", render)
    pal = _render_palette(palette, opt.num_lyt) if render else None
    rend_rec, rend_pred = ([], []) if render else (None, None)
    b, t = real_vid.shape[:2]
    every = list(range(t))
    out = {}
    # reconstruct video (synthesizer.py:436-445).  The reference concatenates all T frames and their layouts
    # (synthesizer.py:445: 2.7 GB per step at the Cityscapes recipe, 1 ms); `decode_output` with `restrict_to_ctx` and no
    # `include_self` reads the CONTEXT frames of it only (lvd.py:716-745, 837; Warper._clip_length): those alone are
    # concatenated -- 29 % of the bytes, the same results bit for bit (tests/test_demo.py compares with the restatement
    # that is handed all T frames)
    n_in = t if getattr(opt, "include_self", False) else ctx_len
    if isinstance(real_vid, WF.PackedClip):
        if real_lyt is not None:
            raise ValueError("predict: a packed clip holds the layout already; pass real_lyt=None")
        real_input = real_vid[:, :n_in]
        ctx_vid = real_vid[:, :ctx_len]  # (the context frames of pred_vid / inp_pred_vid)
        ctx_vid = ctx_vid.rgb() if out_bytes is None else WF.frames_to_bytes(ctx_vid, quantize=out_bytes)
    else:
        real_input = torch.cat([real_vid[:, :n_in], real_lyt[:, :n_in]], dim=2)
        ctx_vid = real_vid[:, :ctx_len]
        if out_bytes is not None:
            ctx_vid = WF.frames_to_bytes(ctx_vid, quantize=out_bytes)
    if getattr(opt, "include_self", False) or not MERGE_DECODES or opt.no_future:
        # the reference's two calls, one after the other (include_self: every frame is a context of itself)
        shared = SharedContext() if not getattr(opt, "include_self", False) else None
        rec, dis, inp, _ = _decode_block(opt, warper, wif, real_input, net, ctx_len, b, every, every, shared=shared,
                                         raw_dtype=raw_dtype, out_bytes=out_bytes, palette=pal, out_render=rend_rec)
        out["rec_vid"], out["rec_disocc"], out["inp_rec_vid"] = rec, dis, inp
        if not opt.no_future:
            alpha = []
            pred, dis, inp, flow = _decode_block(opt, warper, wif, real_input, net, ctx_len, b, every,
                                                 list(range(ctx_len, t)), shared=shared, out_alpha=alpha,
                                                 raw_dtype=raw_dtype, out_bytes=out_bytes, palette=pal,
                                                 out_render=rend_pred)
    else:
        # ONE decode for the reconstruction's and the prediction's units (see decode_units): the context's products once,
        # every full-resolution pass launched once with T + Tp units per clip
        alpha = []
        (rec, dis, inp, _), (pred, dis_p, inp_p, flow) = decode_units(
            opt, warper, wif, real_input, net, ctx_len, b, t, 0, b, every, list(range(ctx_len, t)), out_alpha=alpha,
            raw_dtype=raw_dtype, out_bytes=out_bytes, palette=pal, out_render=rend_rec)
        out["rec_vid"], out["rec_disocc"], out["inp_rec_vid"] = rec, dis, inp
        dis, inp = dis_p, inp_p
        if render:  # (decode_units leaves the reconstruction's pair, then the prediction's)
            rend_pred = [rend_rec.pop()]
    if not opt.no_future:
        # the pose generator (net_pg, outside the path) returns full-length pose sequences: the context
        # poses as they came in, the future ones predicted (flp.py:275-290) -- here the synthetic poses
        # of all T frames stand for them (synthesizer.py:464-472); with the networks: ``predict_future``
        if alpha and alpha[0] is not None:  # (with opt.use_inpainter: what the prediction hands to net_ii.inpaint, synthesizer.py:484)
            out["pred_alpha"] = alpha[0]
        out["pred_disocc"] = dis
        out["pred_flow"] = flow
        out["pred_vid"] = torch.cat([ctx_vid, pred], dim=1)
        out["inp_pred_vid"] = torch.cat([ctx_vid, inp], dim=1)
    if render:
        out["rec_lyt_ids"], out["rec_sem_lyt"] = rend_rec[0]
        if not opt.no_future:
            out["pred_lyt_ids"], out["pred_sem_lyt"] = rend_pred[0]
            out["pred_flow_rgb"] = WR.render_flow(flow, quantize=render)
            if "pred_alpha" in out:
                out["ctx_obj_lyt"] = WR.render_argmax(out["pred_alpha"], WR.layer_palette(out["pred_alpha"].shape[-3]))
    return out


# Synthesizer.predict decodes twice: all T frames from the estimated poses (synthesizer.py:434-445), then the T - Tc future
# frames from the pose generator's (synthesizer.py:464-472).  Both decodes read the same context; their units are
# independent of each other, and the pose generator needs nothing the first decode produces -- so both sets of units can go
# through ONE decode_output on one time axis [context | the reconstruction's other frames | the prediction's frames]: every
# full-resolution pass is launched once with all units (a rank's share of a split job is launch-bound: ~150 launches
# become ~85), what depends on the context alone is computed once by construction.  The same bits per unit (every kernel
# of the chain works per (b, t) unit).  False: the reference's two calls, one after the other.
MERGE_DECODES = True


def decode_units(opt, warper, wif, real_input, net, ctx_len, b, t, b0, b1, rec_frames, pred_frames, out_alpha=None,
                 raw_dtype=None, out_bytes=None, palette=None, out_render=None):
    """The reconstruction's frames ``rec_frames`` and the prediction's frames ``pred_frames`` (clip-relative frame numbers,
    ascending) of clips b0:b1 in ONE decode.  Returns the two 4-tuples of ``_decode_block`` (either may be None when its
    list is empty).  ``raw_dtype``, ``out_bytes``: see ``_decode_block``.  ``out_render`` (a list): receives the
    reconstruction's ``(ids, rgb)`` pair of ``_decode_block``, then the prediction's (views of the one render)."""
    dev = real_input.device
    rec_new = [f for f in rec_frames if f >= ctx_len]
    sel = list(range(ctx_len)) + rec_new + list(pred_frames)
    where = [f if f < ctx_len else ctx_len + rec_new.index(f) for f in rec_frames] + \
            [ctx_len + len(rec_new) + i for i in range(len(pred_frames))]
    blk = _block_net(opt, net, b, t, b0, b1, sel, dev)
    both = [] if out_render is not None else None
    vid, dis, inp, flow = _decode_block(opt, warper, wif, real_input, blk, ctx_len, b1 - b0, sel, where, out_alpha=out_alpha,
                                        raw_dtype=raw_dtype, out_bytes=out_bytes, palette=palette, out_render=both)
    nr = len(rec_frames)
    if both:
        ids, rgb = both[0]
        out_render += [(ids[:, :nr], rgb[:, :nr]), (ids[:, nr:], rgb[:, nr:])]

    def part(lo, hi):
        return (vid[:, lo:hi], dis[:, lo:hi], inp[:, lo:hi], flow[:, :, lo:hi]) if hi > lo else None

    return part(0, nr), part(nr, nr + len(pred_frames))


def rec_unit_order(t, ctx_len):
    """The order in which a clip's T RECONSTRUCTION units are dealt to the ranks (frame numbers).  Two things make units
    unequal: a frame beyond the context costs its rank a control-point grid and a grid inversion of its own (the context
    frames' every rank that shares the clip holds anyway), and a frame far from the context is warped further (larger
    footprint boxes in the frame warp: 1.34 against 1.23 ms per rank and step at the Cityscapes recipe on 8 ranks).
    Dealt in frame order, the rank that got frames 0 .. 6 of a 14-frame clip inverted 7 frames' grids and its neighbour
    11, and the neighbour also predicted the five LATE frames.  Here the context frames are spread evenly among the
    others, and the others are dealt in DESCENDING order: the rank that predicts a clip's early frames (the prediction is
    dealt in frame order) reconstructs its late ones."""
    nc = min(ctx_len, t)
    order, ctx, rest = [], list(range(nc)), list(range(t - 1, nc - 1, -1))
    for i in range(t):  # (a context frame wherever i * nc / t passes an integer)
        if ctx and ((i + 1) * nc // t > i * nc // t or not rest):
            order.append(ctx.pop(0))
        else:
            order.append(rest.pop(0))
    return order


def unit_segments(u0, u1, per_clip, order=None):
    """The units [u0, u1) of a phase's dealing order as runs of clips that decode the SAME frames: [(b0, b1, frames)] --
    a partial first clip, the whole clips in the middle as one batch, a partial last clip.  Unit u is clip u // per_clip,
    position u % per_clip of ``order`` (None: the natural order); ``frames`` are clip-relative unit numbers 0 ..
    per_clip - 1, ASCENDING within a segment -- the order in which ``predict_sharded`` returns them (``local_unit_ids``)."""
    order = list(range(per_clip)) if order is None else list(order)
    segs, u = [], u0
    while u < u1:
        b, i = divmod(u, per_clip)
        if i == 0 and u1 - u >= per_clip:
            nb = (u1 - u) // per_clip
            segs.append((b, b + nb, list(range(per_clip))))
            u += nb * per_clip
        else:
            i1 = min(per_clip, i + (u1 - u))
            segs.append((b, b + 1, sorted(order[i:i1])))
            u += i1 - i
    return segs


def phase_order(phase, t, ctx_len):
    """Dealing order of a phase's per-clip units: reconstruction -> ``rec_unit_order``; prediction -> frame order (every
    predicted frame costs the same)."""
    return rec_unit_order(t, ctx_len) if phase == "rec" else list(range(t - ctx_len))


def local_unit_ids(phase, b, t, ctx_len, rank, world):
    """Natural unit numbers (clip * per_clip + clip-relative unit) of the units ``predict_sharded`` returns for this rank
    and phase, in the order it returns them."""
    from ..dist import shard_range
    per_clip = t if phase == "rec" else t - ctx_len
    u0, u1 = shard_range(b * per_clip, rank, world)
    ids = []
    for b0, b1, frames in unit_segments(u0, u1, per_clip, phase_order(phase, t, ctx_len)):
        ids += [c * per_clip + f for c in range(b0, b1) for f in frames]
    return ids


UNIT_KEYS = {"rec": ("rec_vid", "rec_disocc", "inp_rec_vid"), "pred": ("pred_vid", "pred_disocc", "inp_pred_vid",
                                                                      "pred_flow")}


@torch.no_grad()
def predict_sharded(opt, warper, wif, real_vid, real_lyt, net, ctx_len, rank, world, phases=("rec", "pred"),
                    raw_dtype=None, out_bytes=None, render=None, palette=None):
    """This rank's share of predict() when ONE job (B clips) is split over ``world`` ranks: the
    (b, t) output units of each decode -- B * T reconstructed frames, B * (T - Tc) predicted ones -- are dealt in
    contiguous blocks of the phase's dealing order (dist.shard_range over ``phase_order``: the reconstruction's spreads
    the context frames over the ranks that share a clip, so that every rank inverts the same number of new grids).  A
    rank keeps the context frames of the clips its block touches and their stand-in network outputs, runs the producers
    and Warper.forward for the context frames and ITS frames only, and decodes its block; what depends on a clip's
    context alone (its grids, the layout filter's class distribution, the first occlusion product) is computed ONCE per
    step and clip range (``SharedContext``) and replicated on every rank that shares the clip, which needs no collective.
    Returns {key: (units, C, Hd, Wd)} with the rank's units in the order of ``local_unit_ids``, for the keys of UNIT_KEYS
    (``pred_vid`` / ``inp_pred_vid``: the predicted frames only; ``pred_flow``: Tc * 2 channels); ``gather_predict`` puts
    the ranks' blocks together into predict()'s dict.  Reference: the data-parallel split of tools/engine.py:63-64, here
    over frames instead of clips so that one clip can use every GPU.  ``raw_dtype``, ``out_bytes``: see ``predict`` (with
    ``out_bytes`` the image blocks are uint8 -- a quarter of the bytes the all-gather moves; ``pred_flow`` stays fp32).
    ``render``, ``palette``: see ``predict``; the keys of RENDER_KEYS are added as uint8 unit blocks (the ids with one
    channel, ``pred_flow_rgb`` with Tc * 3)."""
    from ..dist import shard_range
    _check_out_bytes("predict_sharded", out_bytes)
    _check_render("predict_sharded", render)
    pal = _render_palette(palette, opt.num_lyt) if render else None
    if opt.include_self:
        raise ValueError("predict_sharded: include_self appends the predicted frame itself as a context "
                         "(lvd.py:842-845): every rank would need every frame")
    b, t = real_vid.shape[:2]
    dev = real_vid.device
    hd, wd = real_vid.shape[-2:]
    out = {}
    inputs, shared = {}, {}  # clips b0:b1 -> cat of their context frames and layouts / their context's products
    job = (net["raw"], net["pred_obj_pose"], net["pred_bg_pose"], net["occ_score"], net["cls"])
    parts = {k: [] for ph in phases for k in UNIT_KEYS[ph] + (RENDER_KEYS[ph] if render else ())
             if not (ph == "pred" and opt.no_future)}

    def clip_input(b0, b1):
        if (b0, b1) not in inputs:
            inputs[(b0, b1)] = torch.cat([real_vid[b0:b1, :ctx_len], real_lyt[b0:b1, :ctx_len]], dim=2)
            shared[(b0, b1)] = SharedContext()
        return inputs[(b0, b1)]

    def keep(phase, nb, res, rend=None):
        vid, dis, inp, flow = res
        n = vid.shape[1]
        if rend is not None:
            ids, rgb = rend
            parts[phase + "_lyt_ids"].append(ids.reshape(-1, 1, hd, wd))
            parts[phase + "_sem_lyt"].append(rgb.reshape(-1, 3, hd, wd))
            if phase == "pred":  # (nb, Tc, n, 3, Hd, Wd) -> units x (Tc * 3)
                pic = WR.render_flow(flow, quantize=render)
                parts["pred_flow_rgb"].append(pic.permute(0, 2, 1, 3, 4, 5).reshape(nb * n, -1, hd, wd))
        parts[phase + "_vid"].append(vid.reshape(-1, 3, hd, wd))
        parts[phase + "_disocc"].append(dis.reshape(-1, 1, hd, wd))
        parts["inp_" + phase + "_vid"].append(inp.reshape(-1, 3, hd, wd))
        if phase == "pred":  # (nb, Tc, n, 2, Hd, Wd) -> units x (Tc * 2)
            parts["pred_flow"].append(flow.permute(0, 2, 1, 3, 4, 5).reshape(nb * n, -1, hd, wd))

    segs = {}
    for phase in phases:
        if phase == "pred" and opt.no_future:
            continue
        first = 0 if phase == "rec" else ctx_len
        per_clip = t - first
        u0, u1 = shard_range(b * per_clip, rank, world)
        segs[phase] = [(b0, b1, [first + f for f in units])
                       for b0, b1, units in unit_segments(u0, u1, per_clip, phase_order(phase, t, ctx_len))]
    if MERGE_DECODES and len(segs.get("rec", ())) == 1 and len(segs.get("pred", ())) == 1 and \
            segs["rec"][0][:2] == segs["pred"][0][:2]:
        # this rank's reconstruction and prediction units belong to the same clips: ONE decode for both (decode_units)
        b0, b1, rec_frames = segs["rec"][0]
        rend = [] if render else [None, None]
        rec, pred = decode_units(opt, warper, wif, clip_input(b0, b1), net, ctx_len, b, t, b0, b1, rec_frames,
                                 segs["pred"][0][2], raw_dtype=raw_dtype, out_bytes=out_bytes, palette=pal,
                                 out_render=rend if render else None)
        keep("rec", b1 - b0, rec, rend[0])
        keep("pred", b1 - b0, pred, rend[1])
    else:
        for phase, lst in segs.items():
            for b0, b1, frames in lst:
                sel = sorted(set(range(ctx_len)) | set(frames))
                blk = _block_net(opt, net, b, t, b0, b1, sel, dev)
                rend = [] if render else [None]
                res = _decode_block(opt, warper, wif, clip_input(b0, b1), blk, ctx_len, b1 - b0, sel,
                                    [sel.index(f) for f in frames], shared=shared[(b0, b1)],
                                    shared_key=job + (inputs[(b0, b1)],), raw_dtype=raw_dtype, out_bytes=out_bytes,
                                    palette=pal, out_render=rend if render else None)
                keep(phase, b1 - b0, res, rend[0])
    for k, v in parts.items():
        if v:
            out[k] = v[0] if len(v) == 1 else torch.cat(v, dim=0)
        else:  # a rank past the end of a short job holds no unit
            ch = {"disocc": 1, "flow": 2 * (opt.last_n_ctx or ctx_len), "ids": 1}.get(k.split("_")[-1], 3)
            ch = 3 * (opt.last_n_ctx or ctx_len) if k == "pred_flow_rgb" else ch
            as_bytes = (out_bytes is not None and k != "pred_flow") or k in RENDER_KEYS["rec"] + RENDER_KEYS["pred"]
            out[k] = real_vid.new_empty(0, ch, hd, wd, dtype=torch.uint8 if as_bytes else torch.float32)
    return out


def units_to_clips(key, units, b, t, ctx_len, world, real_vid=None, out_bytes=None):
    """The ranks' unit blocks of one key, concatenated in rank order (what the all-gather returns), shaped as predict()
    returns that key: the reconstruction's units go back from dealing order to frame order (one index copy; the
    prediction's are in frame order already), ``pred_flow`` to (B, Tc, Tp, 2, Hd, Wd), the context frames in front of
    ``pred_vid`` / ``inp_pred_vid`` (``real_vid``; with ``out_bytes``, for uint8 units of ``predict_sharded(out_bytes=...)``:
    quantised the same way -- ``real_vid`` the fp32 clip or a ``WF.PackedClip``).  The keys of RENDER_KEYS: the ids lose
    their channel, ``pred_flow_rgb`` goes to (B, Tc, Tp, 3, Hd, Wd)."""
    _check_out_bytes("units_to_clips", out_bytes)
    phase = "rec" if key in UNIT_KEYS["rec"] + RENDER_KEYS["rec"] else "pred"
    per_clip = t if phase == "rec" else t - ctx_len
    if phase == "rec" and world > 1:
        ids = [i for r in range(world) for i in local_unit_ids(phase, b, t, ctx_len, r, world)]
        if ids != list(range(b * per_clip)):
            natural = torch.empty_like(units)
            natural[_cached_index(ids, units.device)] = units
            units = natural
    full = units.view(b, per_clip, *units.shape[1:])
    if key in ("pred_flow", "pred_flow_rgb"):  # units x (Tc * 2 | 3) -> (B, Tc, Tp, 2 | 3, Hd, Wd)
        hd, wd = full.shape[-2:]
        return full.view(b, per_clip, -1, 2 if key == "pred_flow" else 3, hd, wd).permute(0, 2, 1, 3, 4, 5).contiguous()
    if key in ("rec_lyt_ids", "pred_lyt_ids"):
        return full.squeeze(2)
    if key in ("pred_vid", "inp_pred_vid") and real_vid is not None:
        ctx_vid = real_vid[:, :ctx_len]
        if out_bytes is not None:
            ctx_vid = WF.frames_to_bytes(ctx_vid if isinstance(ctx_vid, WF.PackedClip) else ctx_vid[:, :, :3],
                                         quantize=out_bytes)
        return torch.cat([ctx_vid, full], dim=1)
    return full


def gather_predict(local, real_vid, ctx_len, keys=None, group=None, out_bytes=None):
    """All-gather the ranks' blocks of ``predict_sharded`` (one collective per key, ALL issued before the first is waited
    for -- dist.all_gather_frames_async: RCCL over xGMI, or gloo in the tests) and shape them as predict() returns them.
    ``out_bytes``: what ``predict_sharded`` was given (the collectives then move uint8 blocks)."""
    import torch.distributed as dist
    from ..dist import all_gather_frames_async
    b, t = real_vid.shape[:2]
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    keys = list(keys or local.keys())
    pending = {}
    for k in keys:
        per_clip = t if k in UNIT_KEYS["rec"] + RENDER_KEYS["rec"] else t - ctx_len
        pending[k] = all_gather_frames_async(local[k], b * per_clip, group=group)
    return {k: units_to_clips(k, pending[k].wait(), b, t, ctx_len, world, real_vid, out_bytes=out_bytes) for k in keys}


RAW_DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}  # --raw-dtype


def run(clip_dir, out_dir=None, dim=128, aspect_ratio=1.0, num_obj=3, num_lyt=20, frames=6, ctx_len=4, seed=0,
        device="cuda:0", raw_dtype=None, packed=False, eval=False, out_bytes=None, render=None, palette=None,
        wif_ckpt=None, ii_depth=4, ii_embed_dim=512, unet_dtype=None, lpips=None):
    """The demo on a clip directory.  ``packed``: the clip goes to the device packed (RGB bytes + class ids,
    ``WF.PackedClip``) and predict() reads it as such -- the same results.  ``eval``: also score ``rec_vid`` and
    ``inp_pred_vid`` against the real frames (``evaluate_prediction``; with ``lpips``, an ``LPIPS`` module on the device,
    LPIPS too -- not with ``packed``), returned under ``"metrics"``.  ``out_bytes``
    ("trunc" / "round"): predict() returns its clips as uint8, and those bytes are what is written and scored.
    ``render`` ("trunc" / "round"), ``palette`` (3 * num_lyt integers): predict()'s renders of the decomposition; the
    layout pictures, the flow picture of the last context and ``ctx_obj_lyt`` are written as ``.gif`` + ``_last.png``.
    ``wif_ckpt``: a reference ``ii`` state dict (``load_wif_checkpoint``) run through ``WIF.with_unet`` at ``ii_depth`` /
    ``ii_embed_dim`` in place of the stand-in network; ``unet_dtype`` (torch.bfloat16 / torch.float16): with 16-bit
    activations (``UNet.act_dtype``) -- with the same ``raw_dtype`` the chain from ``raw_output`` to the fusion kernel is
    16-bit throughout, no fp32 copy of ``raw_output`` or of a level's activations is made."""
    if unet_dtype is not None and wif_ckpt is None:
        raise ValueError("demo.run: unet_dtype needs wif_ckpt (the stand-in network has no activations to store)")
    opt = demo_opt(dim, aspect_ratio, num_obj, num_lyt, ctx_len=ctx_len, ii_depth=ii_depth, ii_embed_dim=ii_embed_dim)
    size = (dim, int(dim * aspect_ratio))
    clip = wio.load_clip(clip_dir, size, num_lyt, max_frames=frames, packed=packed)
    dev = torch.device(device)
    if packed:
        vid, lyt = clip["vid"].to(dev), None
    else:
        vid, lyt = clip["vid"].unsqueeze(0).to(dev), clip["lyt"].unsqueeze(0).to(dev)
    warper = Warper(opt).to(dev)
    if wif_ckpt is not None:
        wif = load_wif_checkpoint(WIF.with_unet(opt, act_dtype=unet_dtype), wif_ckpt).to(dev).eval()
    else:
        wif = WIF(opt, unet=UniformFusionUNet()).to(dev)
    net = synthetic_network_outputs(opt, 1, vid.shape[1], ctx_len, seed=seed, device=dev)
    res = predict(opt, warper, wif, vid, lyt, net, ctx_len, raw_dtype=raw_dtype, out_bytes=out_bytes, render=render,
                  palette=palette)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        pics = {key: res[key][0] for key in ("rec_sem_lyt", "pred_sem_lyt") if key in res}
        if "pred_flow_rgb" in res:
            pics["pred_flow_rgb"] = res["pred_flow_rgb"][0, -1]  # (the last context's flows)
        if "ctx_obj_lyt" in res:
            pics["ctx_obj_lyt"] = res["ctx_obj_lyt"][0].reshape(-1, *res["ctx_obj_lyt"].shape[-3:])
        for key, pic in pics.items():  # (uint8 already: written as they are)
            wio.dump_video(pic.cpu(), os.path.join(out_dir, key + ".gif"))
            wio.dump_image(pic[-1].cpu(), os.path.join(out_dir, key + "_last.png"))
        for key in ("rec_vid", "inp_rec_vid", "pred_vid", "inp_pred_vid"):
            if key in res:
                wio.dump_video(res[key][0], os.path.join(out_dir, key + ".gif"))
                wio.dump_image(res[key][0, -1], os.path.join(out_dir, key + "_last.png"))
        if "pred_flow" in res:
            fl = res["pred_flow"][0, -1, 0]
            wio.write_flo(os.path.join(out_dir, "pred_flow_last.flo"), fl)
    if eval:
        res["metrics"] = evaluate_prediction(res, vid, lpips=lpips)
    return res


def load_wif_checkpoint(wif, path):
    """Load a reference ``ii`` state dict (the file, or a tensor-only dict in it under "state_dict") into ``wif``
    (``WIF.with_unet``), strictly; a ``module.`` prefix (DistributedDataParallel) is stripped."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state:
        state = state["state_dict"]
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    wif.load_state_dict(state, strict=True)
    return wif


def load_lvd_checkpoint(lvd, path):
    """Load a reference ``pe`` state dict (the file, or a tensor-only dict in it under "state_dict") into ``lvd``
    (``nets.LVD`` built from the checkpoint's options), strictly; a ``module.`` prefix is stripped."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state:
        state = state["state_dict"]
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    lvd.load_state_dict(state, strict=True)
    return lvd


def load_flp_checkpoint(flp, path):
    """Load a reference ``pg`` state dict (the file, or a tensor-only dict in it under "state_dict") into ``flp``
    (``nets.FLP`` built from the checkpoint's options), strictly; a ``module.`` prefix is stripped."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state:
        state = state["state_dict"]
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    flp.load_state_dict(state, strict=True)
    return flp


def flp_demo_opt(nopt, **over):
    """``nets.flp_net_opt`` next to LVD networks built from ``nopt``: the fields the two share (token rasters, width,
    heads, objects, the pose heads' constants) taken from ``nopt``, FLP's own (depths, ``pg_num_timesteps``, ``cat_z``,
    ...: the checkpoint's training options) from ``over``."""
    from ..nets.flp import flp_net_opt
    known = vars(flp_net_opt())
    d = {k: v for k, v in vars(nopt).items() if k in known}
    d.update(over)
    return flp_net_opt(**d)


def lvd_demo_opt(opt, **over):
    """``nets.lvd_net_opt`` for the demo's ``opt``: the fields the two share taken from ``opt``, the networks' own
    (widths, depths, input modalities: the checkpoint's training options) from ``over``."""
    from ..nets.lvd import lvd_net_opt
    known = vars(lvd_net_opt())
    d = {k: v for k, v in vars(opt).items() if k in known}
    d["time_dropout"] = False
    d.update(over)
    nopt = lvd_net_opt(**d)
    # the encoder's token raster is the frame over scale_factor over patch_size: it has to be latent_shape
    raster = [int(nopt.dim / nopt.scale_factor) // nopt.patch_size,
              int(nopt.dim * nopt.aspect_ratio / nopt.scale_factor) // nopt.patch_size]
    if raster != list(nopt.latent_shape):
        raise ValueError(f"lvd_demo_opt: {nopt.dim} x {int(nopt.dim * nopt.aspect_ratio)} frames at scale_factor "
                         f"{nopt.scale_factor} and patch_size {nopt.patch_size} give {raster} tokens, latent_shape is "
                         f"{list(nopt.latent_shape)}")
    return nopt


def reconstruct(opt, lvd, wif, real_vid, real_lyt, real_flow, ctx_len):
    """The reconstruction half of the reference's ``Synthesizer.predict`` (models/synthesizer.py:419-460) with the
    decomposition coming from the networks: encode the clip, estimate the layers from the first ``ctx_len`` frames, the
    poses of every frame, alphas / grids / occlusion, decode every frame from the context frames and fuse.  ``opt``:
    the options ``lvd`` was built from (input_rgb / input_lyt / input_flow, last_n_ctx if present).  real_vid
    (B, T, 3, H, W), real_lyt (B, T, Nl, H, W), real_flow (B, T, 2, H, W) or None when ``opt.input_flow`` is off.
    Returns ``rec_vid``, ``rec_disocc``, ``inp_rec_vid`` and the decomposition (``cls``, ``obj_pose``, ``bg_pose``,
    ``occ``, ``obj_alpha``)."""
    with torch.no_grad():
        parts = [real_vid] if opt.input_rgb else []
        parts += [real_lyt] if opt.input_lyt else []
        if opt.input_flow:
            if real_flow is None:
                raise ValueError("reconstruct: the networks take the flow as input (opt.input_flow) and real_flow is None")
            parts.append(real_flow)
        x = lvd(input=torch.cat(parts, dim=2), mode="encode_input")
        x_obj, x_bg, cls = lvd(x=x[:, :ctx_len], mode="estimate_layer")
        obj_pose, bg_pose, occ_score = lvd(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")[:3]
        occ, obj_alpha, bg_alpha, grid = lvd(x_obj=x_obj, obj_pose=obj_pose, bg_pose=bg_pose, occ_score=occ_score,
                                             mode="estimate_alpha_grid_occ")
        b, t = x.shape[:2]
        ctx_ts = torch.arange(ctx_len, device=x.device, dtype=torch.int64).view(1, -1, 1).expand(b, -1, t)
        if getattr(opt, "last_n_ctx", 0) > 0:
            ctx_ts = ctx_ts[:, -opt.last_n_ctx:]
        pred_ts = torch.arange(t, device=x.device, dtype=torch.int64)
        out = lvd(input=torch.cat([real_vid, real_lyt], dim=2), grid=grid, occ=occ, obj_alpha=obj_alpha, bg_alpha=bg_alpha,
                  ctx_ts=ctx_ts.contiguous(), pred_ts=pred_ts, cls=cls, mode="decode_output")
        rec_output, raw_output, alpha_ctx = out[0], out[5], out[6]
        disocc = WF.disocc_test(alpha_ctx.amax(dim=3))  # synthesizer.py:447-450
        return dict(rec_vid=rec_output[:, :, :3], rec_disocc=disocc.unsqueeze(2), inp_rec_vid=wif(raw_output), cls=cls,
                    obj_pose=obj_pose, bg_pose=bg_pose, occ=occ, obj_alpha=obj_alpha)


def predict_future(opt, lvd, flp, wif, real_vid, real_lyt, real_flow, ctx_len):
    """The prediction half of the reference's ``Synthesizer.predict`` (models/synthesizer.py:462-480) with the poses of
    the frames after the first ``ctx_len`` coming from FLP: the decomposition of ``reconstruct``, FLP on the poses of
    the whole clip under the mask "the first ``ctx_len`` frames" -- an integer-built plan, so nothing of it reads the
    host --, alphas / grids / occlusion for the predicted poses, the future frames decoded from the context frames and
    fused.  Arguments as ``reconstruct``; ``flp``: ``nets.FLP`` of the same widths and rasters as ``lvd``.  Returns
    ``pred_vid`` (B, T, 3, H, W: the context frames as they are, then the predicted ones), ``fused_pred_vid``
    (B, T - ctx_len, 3, H, W: ``wif`` on the raw output; the reference's border inpainting is ``WIF.inpaint``),
    ``pred_disocc`` and the poses FLP returned (``obj_pose``, ``bg_pose``, ``occ_score``: all T frames)."""
    with torch.no_grad():
        parts = [real_vid] if opt.input_rgb else []
        parts += [real_lyt] if opt.input_lyt else []
        if opt.input_flow:
            if real_flow is None:
                raise ValueError("predict_future: the networks take the flow as input (opt.input_flow) and real_flow is "
                                 "None")
            parts.append(real_flow)
        x = lvd(input=torch.cat(parts, dim=2), mode="encode_input")
        b, t = x.shape[:2]
        if not 0 < ctx_len < t:
            raise ValueError(f"predict_future: 0 < ctx_len < {t} frames, got {ctx_len}")
        x_obj, x_bg, cls = lvd(x=x[:, :ctx_len], mode="estimate_layer")
        obj_pose, bg_pose, occ_score, _, _, last_obj, last_bg = lvd(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")
        obj_pose, bg_pose, occ_score = flp(obj_pose, bg_pose, occ_score, x_obj, x_bg, last_obj, last_bg,
                                           ctx_mask=flp.plan(b, t, ctx_len, x.device))
        occ, obj_alpha, bg_alpha, grid = lvd(x_obj=x_obj, obj_pose=obj_pose, bg_pose=bg_pose, occ_score=occ_score,
                                             mode="estimate_alpha_grid_occ")
        pred_ts = torch.arange(ctx_len, t, device=x.device, dtype=torch.int64)
        ctx_ts = torch.arange(ctx_len, device=x.device, dtype=torch.int64).view(1, -1, 1).expand(b, -1, t - ctx_len)
        out = lvd(input=torch.cat([real_vid, real_lyt], dim=2), grid=grid, occ=occ, obj_alpha=obj_alpha, bg_alpha=bg_alpha,
                  ctx_ts=ctx_ts.contiguous(), pred_ts=pred_ts, cls=cls, mode="decode_output")
        pred_output, raw_output, alpha_ctx = out[0], out[5], out[6]
        disocc = WF.disocc_test(alpha_ctx.amax(dim=3))  # synthesizer.py:474-477
        return dict(pred_vid=torch.cat([real_vid[:, :ctx_len], pred_output[:, :, :3]], dim=1),
                    fused_pred_vid=wif(raw_output), pred_disocc=disocc.unsqueeze(2), obj_pose=obj_pose, bg_pose=bg_pose,
                    occ_score=occ_score)


def run_lvd(clip_dir, lvd_ckpt, out_dir=None, dim=128, aspect_ratio=1.0, num_obj=3, num_lyt=20, frames=6, ctx_len=4,
            device="cuda:0", lvd_over=None, wif_ckpt=None, ii_depth=4, ii_embed_dim=512, flp_ckpt=None, flp_over=None,
            nets_dtype=None):
    """``--lvd-ckpt``: the clip through ``reconstruct`` with a reference ``pe`` checkpoint; ``rec_vid`` and
    ``inp_rec_vid`` written by the writers ``run`` uses.  ``lvd_over``: the checkpoint's training options where they
    differ from ``lvd_demo_opt(demo_opt(...))`` (``--lvd-opt FILE``: a JSON object).  ``flp_ckpt`` (``--flp-ckpt``): a
    reference ``pg`` checkpoint too -- the frames after ``ctx_len`` through ``predict_future`` as well (``pred_vid``,
    ``fused_pred_vid``); ``flp_over``: its training options where they differ from ``flp_demo_opt`` (``--flp-opt``).
    ``nets_dtype`` (``--nets-dtype``; torch.bfloat16 / torch.float16): the ``act_dtype`` of the LVD and FLP networks --
    under autocast with the 16-bit attention kernel; the warp path stays fp32."""
    from ..nets.flp import FLP
    from ..nets.lvd import LVD
    opt = demo_opt(dim, aspect_ratio, num_obj, num_lyt, ctx_len=ctx_len, ii_depth=ii_depth, ii_embed_dim=ii_embed_dim)
    nopt = lvd_demo_opt(opt, **(lvd_over or {}))
    dev = torch.device(device)
    clip = wio.load_clip(clip_dir, (dim, int(dim * aspect_ratio)), num_lyt, max_frames=frames)
    vid, lyt = clip["vid"].unsqueeze(0).to(dev), clip["lyt"].unsqueeze(0).to(dev)
    flow = None
    if nopt.input_flow:
        if clip.get("flow") is None:
            raise ValueError(f"run_lvd: the networks take the flow as input and {clip_dir} has no flow files next to it")
        flow = torch.nn.functional.interpolate(clip["flow"].to(dev), size=vid.shape[-2:], mode="bilinear").unsqueeze(0)
    lvd = load_lvd_checkpoint(LVD(nopt), lvd_ckpt).to(dev).eval()
    lvd.act_dtype = nets_dtype
    if wif_ckpt is not None:
        wif = load_wif_checkpoint(WIF.with_unet(opt), wif_ckpt).to(dev).eval()
    else:
        wif = WIF(opt, unet=UniformFusionUNet()).to(dev)
    res = reconstruct(nopt, lvd, wif, vid, lyt, flow, ctx_len)
    keys = ("rec_vid", "inp_rec_vid")
    if flp_ckpt is not None:
        flp = load_flp_checkpoint(FLP(flp_demo_opt(nopt, **(flp_over or {}))), flp_ckpt).to(dev).eval()
        flp.act_dtype = nets_dtype
        future = predict_future(nopt, lvd, flp, wif, vid, lyt, flow, ctx_len)
        res.update(pred_vid=future["pred_vid"], fused_pred_vid=future["fused_pred_vid"])
        keys += ("pred_vid", "fused_pred_vid")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        for key in keys:
            wio.dump_video(res[key][0], os.path.join(out_dir, key + ".gif"))
            wio.dump_image(res[key][0, -1], os.path.join(out_dir, key + "_last.png"))
    return res


EVAL_KEYS = ("rec_vid", "inp_pred_vid")


def evaluate_prediction(res, real_vid, lpips=None):
    """PSNR / SSIM / MS-SSIM (and, with an ``LPIPS`` module and a dense ``real_vid``, LPIPS) of ``rec_vid`` and ``inp_pred_vid`` against the real frames at the same time indices, both
    quantised to the bytes the reference dumps (its two save_vid calls: ``metrics.frame_metrics``'s "trunc").  ``real_vid``:
    the fp32 clip (B, T, 3, H, W) or the ``WF.PackedClip``.  MS-SSIM is left out below its size limit (161 x 161).
    Returns {key: {metric: (B, T) tensor}}."""
    from .. import metrics as M
    h, w = real_vid.shape[-2:]
    names = tuple(m for m in M.METRICS if m != "msssim" or min(h, w) >= M.MIN_MSSSIM_SIDE)
    if lpips is not None:
        names += ("lpips",)
    real = real_vid if isinstance(real_vid, WF.PackedClip) else real_vid[:, :, :3]
    return {key: M.frame_metrics(res[key], real, metrics=names, lpips=lpips) for key in EVAL_KEYS if key in res}


def print_evaluation(scores, ctx_len, frame_size):
    from .. import metrics as M
    if min(frame_size) < M.MIN_MSSSIM_SIDE:
        print(f"msssim: not applicable at {frame_size[0]}x{frame_size[1]} (needs {M.MIN_MSSSIM_SIDE}x{M.MIN_MSSSIM_SIDE})")
    for key, sc in scores.items():
        print(f"{key}:")
        for line in M.format_lines(M.summarize(sc, ctx_len)):
            print(line)


def read_palette_file(path):
    """``--palette FILE``: integers separated by white space or commas (3 per layout class), as a flat list."""
    with open(path) as fh:
        return [int(v) for v in fh.read().replace(",", " ").split()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--clip", required=True, help="directory with the clip's frame PNGs (demo dataset layout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--aspect-ratio", type=float, default=1.0)
    ap.add_argument("--num-obj", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--ctx-len", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--raw-dtype", choices=sorted(RAW_DTYPES), default="fp32",
                    help="element type of the WIF input raw_output (bf16 / fp16: what a UNet under autocast takes)")
    ap.add_argument("--packed", action="store_true",
                    help="hand the clip over packed: RGB bytes + class ids, 4 bytes per pixel (the same results)")
    ap.add_argument("--bytes", choices=sorted(WF.BYTE_QUANTIZE), default=None, dest="out_bytes",
                    help="return and write the clips as bytes quantised on the device (trunc: the reference's "
                         "dump_video; round: this package's)")
    ap.add_argument("--render", nargs="?", const="trunc", choices=sorted(WR.QUANTIZE), default=None,
                    help="also render the decomposition on the device: layout class ids and pictures, the flow wheel "
                         "(the value: the quantisation of the flow picture)")
    ap.add_argument("--palette", default=None, metavar="FILE",
                    help="with --render: a text file of 3 * num_lyt integers, the layout colours (default: the jet "
                         "colours of the object layers)")
    ap.add_argument("--eval", action="store_true",
                    help="score rec_vid and inp_pred_vid against the real frames (PSNR, SSIM, MS-SSIM from 161x161)")
    from .evaluate import LPIPS_DTYPES, add_lpips_arguments, lpips_module
    add_lpips_arguments(ap)  # (with --eval, and not with --packed: LPIPS takes dense clips)
    ap.add_argument("--wif-ckpt", default=None, metavar="FILE",
                    help="a reference `ii` checkpoint (state dict): run the reference's UNet (WIF.with_unet) in place of "
                         "the stand-in network")
    ap.add_argument("--unet-dtype", choices=sorted(RAW_DTYPES), default="fp32",
                    help="with --wif-ckpt: the element type of the UNet's activations (bf16 / fp16: under autocast, the "
                         "norm + GELU kernel included; with the same --raw-dtype nothing in between is fp32)")
    ap.add_argument("--ii-depth", type=int, default=4, help="with --wif-ckpt: the checkpoint's --s_ii_depth")
    ap.add_argument("--ii-embed-dim", type=int, default=512, help="with --wif-ckpt: the checkpoint's --s_ii_embed_dim")
    ap.add_argument("--lvd-ckpt", default=None, metavar="FILE",
                    help="a reference `pe` checkpoint (state dict): decompose the clip with the LVD networks and write "
                         "its reconstruction (rec_vid, inp_rec_vid) instead of running the seeded stand-ins")
    ap.add_argument("--lvd-opt", default=None, metavar="FILE",
                    help="with --lvd-ckpt: a JSON object of the checkpoint's training options (embed_dim, num_heads, "
                         "oe_depth, pe_depth, input_lyt, ...) where they differ from the defaults")
    ap.add_argument("--flp-ckpt", default=None, metavar="FILE",
                    help="with --lvd-ckpt: a reference `pg` checkpoint (state dict): predict the frames after --ctx-len "
                         "with the FLP networks and write them too (pred_vid, fused_pred_vid)")
    ap.add_argument("--flp-opt", default=None, metavar="FILE",
                    help="with --flp-ckpt: a JSON object of the checkpoint's training options (pg_enc_depth, "
                         "pg_num_timesteps, cat_z, ...) where they differ from the defaults")
    ap.add_argument("--nets-dtype", choices=sorted(RAW_DTYPES), default="fp32",
                    help="with --lvd-ckpt: the element type of the LVD / FLP networks' activations (bf16 / fp16: under "
                         "autocast, with the 16-bit token attention kernel; poses, grids and the warp path stay fp32)")
    args = ap.parse_args()
    if args.nets_dtype != "fp32" and args.lvd_ckpt is None:
        ap.error("--nets-dtype needs --lvd-ckpt: the seeded stand-ins have no networks")
    if args.flp_ckpt is not None and args.lvd_ckpt is None:
        ap.error("--flp-ckpt needs --lvd-ckpt: FLP predicts the poses the LVD networks estimate")
    if args.lvd_ckpt is not None:
        import json
        over = {}
        for name in ("lvd_opt", "flp_opt"):
            if getattr(args, name) is not None:
                with open(getattr(args, name)) as fh:
                    over[name] = json.load(fh)
        res = run_lvd(args.clip, args.lvd_ckpt, args.out, args.dim, args.aspect_ratio, args.num_obj, frames=args.frames,
                      ctx_len=args.ctx_len, lvd_over=over.get("lvd_opt"), wif_ckpt=args.wif_ckpt, ii_depth=args.ii_depth,
                      ii_embed_dim=args.ii_embed_dim, flp_ckpt=args.flp_ckpt, flp_over=over.get("flp_opt"),
                      nets_dtype=RAW_DTYPES[args.nets_dtype])
        for k, v in res.items():
            if v is not None:
                print(f"{k}: {tuple(v.shape)} range [{v.min().item():.3f}, {v.max().item():.3f}] "
                      f"finite={bool(torch.isfinite(v).all())}")
        return
    palette = read_palette_file(args.palette) if args.palette is not None else None
    res = run(args.clip, args.out, args.dim, args.aspect_ratio, args.num_obj, frames=args.frames,
              ctx_len=args.ctx_len, seed=args.seed, raw_dtype=RAW_DTYPES[args.raw_dtype], packed=args.packed,
              eval=args.eval, out_bytes=args.out_bytes, render=args.render, palette=palette, wif_ckpt=args.wif_ckpt,
              ii_depth=args.ii_depth, ii_embed_dim=args.ii_embed_dim, unet_dtype=RAW_DTYPES[args.unet_dtype],
              lpips=lpips_module(args.lpips_net, args.lpips_state, args.lpips_backbone, args.lpips_lin,
                                 act_dtype=LPIPS_DTYPES[args.lpips_dtype]) if args.eval else None)
    scores = res.pop("metrics", None)
    for k, v in res.items():
        print(f"{k}: {tuple(v.shape)} range [{v.min().item():.3f}, {v.max().item():.3f}] "
              f"finite={bool(torch.isfinite(v).all())}")
    if scores is not None:
        print_evaluation(scores, args.ctx_len, tuple(res["rec_vid"].shape[-2:]))


if __name__ == "__main__":
    main()
