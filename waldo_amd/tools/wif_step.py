"""The warp-path part of one WIF training step as the reference runs it -- BASELINE config 3's real call order
(``Synthesizer.inpaint``, models/synthesizer.py:517-576, 631-633, at scripts/cityscapes/train_wif.sh: 8 clips over 4
GPUs = 2 clips per GPU, ``vid_len 5`` with ``ctx_len 4`` -> one predicted frame, 16 objects + background, 20 layout
classes, 128 x 256 layers, 512 x 1024 frames):

    under torch.no_grad():   decoder tail -> pose heads' affine -> estimate_alpha_grid_occ (synthesizer.py:532)
                             real_input = cat([real_vid, real_lyt])                        (synthesizer.py:535)
                             decode_output with ctx_ts = 0 .. 3, pred_ts = [4]             (synthesizer.py:568-573)
                             -- train_wif.sh does NOT pass --s_restrict_to_ctx: the UNRESTRICTED Warper.grid_to_flow
                             (lvd.py:602-705: alphas composited on all T frames), then input_to_output
    with autograd:           inp_output = net_ii(raw_output)  = WIF.forward                (synthesizer.py:576)
                             loss (the `sharp_vid` L1 term, synthesizer.py:587-590), backward (synthesizer.py:631)

The networks outside the path are stand-ins: seeded decoder logits / pose head outputs / occlusion scores / class
distributions, and a 1 x 1 convolution (40 -> 5 channels, the UNet's widths at ``ii_score`` + ``ii_ab``, wif.py:19-23)
in the UNet's place so that ``waldo_wif_fuse_bwd`` receives and produces real gradients.  ``bench.py --config WIF``
times it.  ``WifStep(..., unet="reference")`` puts the real network there (``WIF.with_unet`` at the recipe's widths:
``ii_depth 6``, ``ii_embed_dim 512``); ``act_dtype`` runs it with 16-bit activations (``UNet.act_dtype``).  ``WifStep(..., objective="recipe")`` runs the recipe's full objective,
``--s_vid_inpainting_losses "sharp_vid" "lpips_vid"`` with both lambdas 1 (synthesizer.py:587-600): the L1 term plus
``LPIPS("vgg")`` of the predicted frames against the real ones (``nets.lpips``; random weights unless a module is passed).
With ``unet="reference"``, ``optimizer="adam"`` / ``"adamw"`` / an ``optim.Adam`` ends the step as the reference does
(synthesizer.py:619-631) with ``optimizer.step(loss)`` on the device (``waldo_amd.optim``); None stops at the gradients.
"""
import torch
import torch.nn as nn

from .. import functional as WF
from .. import optim
from ..nets import LPIPS, WIF, Warper, decode_output, estimate_alpha_grid_occ, flp
from ..nets.lvd import decoder_tail
from . import demo
from .pipeline import synthetic_clip


def wif_opt(**over):
    """The option fields the path reads, at the Cityscapes WIF recipe (train_wif.sh:12-16, 25-37)."""
    d = dict(dim=128, aspect_ratio=2.0, num_obj=16, num_lyt=20, load_dim=512, latent_shape=[8, 16], obj_shape=[4, 4],
             patch_size=16, scale_factor=1, min_cls=0.1, use_lyt_opacity=True, pad_obj_alpha=3, ii_depth=6)
    d.update(over)
    return demo.demo_opt(**d)


class WifStep:
    """``clips`` clips of 5 frames resident on ``device``; ``__call__`` runs the no-grad decode, ``WIF.forward``, the
    loss and its backward once and returns the loss (the stand-in network's ``.grad`` hold the gradients).
    ``objective``: ``"sharp"``, the `sharp_vid` L1 term alone, or ``"recipe"``, `sharp_vid` + `lpips_vid` as train_wif.sh
    trains; ``lpips``: the ``LPIPS`` module of the latter (a seeded random-weight ``LPIPS("vgg")`` when None);
    ``lpips_dtype``: that module's ``act_dtype`` (bf16 / fp16 backbone activations and the 16-bit level kernels; a given
    ``lpips`` must agree with it).  After a
    call ``terms`` holds the detached terms of the loss by the reference's names.  ``opt_over``: option fields that differ
    from the recipe's (a smaller UNet: ``ii_embed_dim``, ``ii_depth``; smaller frames: ``load_dim``).  ``optimizer`` (with ``unet="reference"``): None,
    "adam", "adamw" or an ``optim.Adam`` over the UNet's parameters; the step then ends in ``optimizer.step(loss)``, and
    ``step.optimizer`` is it."""

    frames, ctx_len = 5, 4

    def __init__(self, clips, device, seed=0, motion="calibrated", unet="stand-in", act_dtype=None, objective="sharp",
                 lpips=None, optimizer=None, opt_over=None, lpips_dtype=None):
        if optimizer is not None and unet != "reference":
            raise ValueError("WifStep: optimizer= needs unet='reference' (the stand-in is not the network that trains)")
        if objective not in ("sharp", "recipe"):
            raise ValueError(f"WifStep: objective must be 'sharp' or 'recipe', got {objective!r}")
        if lpips is not None and objective != "recipe":
            raise ValueError("WifStep: lpips= needs objective='recipe' (the 'sharp' objective has no LPIPS term)")
        if lpips is not None and not isinstance(lpips, LPIPS):
            raise ValueError(f"WifStep: lpips must be an LPIPS module, got {type(lpips).__name__}")
        if lpips_dtype is not None and objective != "recipe":
            raise ValueError("WifStep: lpips_dtype= needs objective='recipe' (the 'sharp' objective has no LPIPS term)")
        if lpips_dtype is not None and lpips is not None and lpips.act_dtype != lpips_dtype:
            raise ValueError(f"WifStep: lpips_dtype={lpips_dtype} disagrees with the given module's act_dtype="
                             f"{lpips.act_dtype}")
        if unet not in ("stand-in", "reference"):
            raise ValueError(f"WifStep: unet must be 'stand-in' or 'reference', got {unet!r}")
        if act_dtype is not None and unet != "reference":
            raise ValueError("WifStep: act_dtype needs unet='reference' (the stand-in has no activations to store)")
        self.opt = o = wif_opt(**(opt_over or {}))
        self.clips, self.device = clips, device
        self.warper = Warper(o).to(device)
        torch.manual_seed(seed)
        if unet == "reference":
            self.wif = WIF.with_unet(o, act_dtype=act_dtype).to(device)
            self.unet = self.wif.unet
        else:
            self.unet = nn.Conv2d(3 + o.num_lyt + o.num_obj + 1, 5, 1).to(device)
            self.wif = WIF(o, unet=self.unet).to(device)
        self.optimizer = optim.resolve(optimizer, list(self.unet.parameters()), "WifStep")
        self.net = demo.synthetic_network_outputs(o, clips, self.frames, self.ctx_len, seed=seed, device=device,
                                                  motion=motion)
        self.vid, self.lyt = synthetic_clip(o, clips, self.frames, seed, device)
        t, tc = self.frames, self.ctx_len
        # synthesizer.py:568-570: the context frames' indices, expanded over the predicted frames; the predicted frame
        self.ctx_ts = torch.arange(tc, device=device, dtype=torch.int64).view(1, -1, 1).expand(clips, -1, t - tc).contiguous()
        self.pred_ts = torch.arange(tc, t, device=device, dtype=torch.int64)
        self.raw_output = None
        self.objective, self.terms, self.lpips = objective, {}, None
        if objective == "recipe":
            if lpips is None:
                # (no global generator is touched; a bad lpips_dtype is LPIPS's ValueError)
                lpips = LPIPS("vgg", generator=torch.Generator().manual_seed(seed), act_dtype=lpips_dtype)
            self.lpips = lpips.to(device)

    def decode(self):
        """The no-grad half: what ``inpaint`` computes before ``net_ii`` (synthesizer.py:517-574)."""
        o, b, t = self.opt, self.clips, self.frames
        no = o.num_obj
        lo, lb = o.obj_shape[0] * o.obj_shape[1], o.latent_shape[0] * o.latent_shape[1]
        dev = self.device
        net = self.net
        with torch.no_grad():
            buf = demo.pose_buffers(o, dev)
            bg_alpha = demo._cached("bg_alpha", o, dev, lambda: torch.ones(1, 1, o.dim, int(o.dim * o.aspect_ratio), device=dev))
            obj_pose = flp.obj_pose_to_points(net["pred_obj_pose"], buf["tgt_pts_obj"], buf["mul_obj"], buf["bias_obj"])
            bg_pose = flp.bg_pose_to_points(net["pred_bg_pose"], buf["tgt_pts_bg"], buf["bias_bg"])
            obj_alpha = decoder_tail(net["raw"], init_bias=0.0, scale_factor=o.scale_factor)
            obj_alpha = obj_alpha.view(b, no, 1, *obj_alpha.shape[-2:])
            occ, obj_alpha, bga, grid = estimate_alpha_grid_occ(self.warper, obj_alpha, bg_alpha,
                                                                obj_pose.view(b, t, no, lo, 2), bg_pose.view(b, t, 1, lb, 2),
                                                                net["occ_score"], obj_alpha_mask=demo.obj_alpha_mask(o, dev))
            real_input = torch.cat([self.vid, self.lyt], dim=2)  # (all T frames: the unrestricted path composites on them)
            out = decode_output(self.warper, real_input, grid, occ, obj_alpha, bga, net["cls"], self.ctx_ts,
                                self.pred_ts, restrict_to_ctx=False)
        return out  # (output, flow, alpha_unflt, alpha, raw_alpha, raw_output, alpha_ctx)

    def __call__(self):
        for p in self.unet.parameters():
            p.grad = None
        rec_output, _, _, _, _, raw_output, _ = self.decode()
        self.raw_output = raw_output
        inp_output = self.wif(raw_output)                                   # synthesizer.py:576
        real = self.vid[:, self.ctx_len:]
        loss = (inp_output[:, :, :3] - real).abs().mean()                   # `sharp_vid` (synthesizer.py:587-590)
        self.terms = {"sharp_vid": loss.detach()}
        if self.objective == "recipe":                                      # `lpips_vid` (synthesizer.py:597-600)
            lp = self.lpips(inp_output[:, :, :3].flatten(0, 1), real.flatten(0, 1)).mean()
            self.terms["lpips_vid"] = lp.detach()
            loss = loss + lp
        loss.backward()                                                     # synthesizer.py:631
        if self.optimizer is not None:
            self.optimizer.step(loss.detach())
        return loss

    def grads_finite(self):
        return all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in self.unet.parameters())

    def hd_algorithmic_bytes(self):
        """Bytes the full-resolution entry points have to move per step (each input read once, each output written
        once; fp32), by C-ABI name -- as ``Pipeline.hd_algorithmic_bytes``, for the UNRESTRICTED flow synthesis (the
        first pass composites on all T frames and writes ``alpha`` as well: ``inpaint`` keeps it in the tuple)."""
        o = self.opt
        b, t, tc = self.clips, self.frames, self.ctx_len
        tp = t - tc
        nl, ncls, c = o.num_obj + 1, o.num_lyt, 3 + o.num_lyt
        hw = o.dim * int(o.dim * o.aspect_ratio)
        hwd = o.load_dim * int(o.load_dim * o.aspect_ratio)
        m, u = b * tc * tp, b * tp
        lr = m * (nl * 2) * hw                                   # per-layer flows (no ghost mask on this path)
        return {
            "waldo_flow_ctx_alpha_fwd": 4 * (b * t * nl * hw + b * t * ncls * hwd + 2 * b * t * nl * hwd),
            "waldo_flow_ctx_warp_raw_fwd": 4 * (lr + b * tc * nl * hwd + m * (2 + nl + 1) * hwd + m * hwd),
            "waldo_frame_warp_fuse_raw_fwd": 4 * (b * tc * c * hwd + m * (2 + 1) * hwd + u * (c + 1) * hwd + m * c * hwd),
            "waldo_wif_fuse_fwd": 4 * (m * 4 * hwd + m * 4 * hwd + u * 3 * hwd),
            # reads vid channels 0-2 and 4, the network's 4 used outputs, out and grad_out; writes all 5 planes of
            # grad_net per (unit, context) (raw_output carries no gradient: grad_vid is not produced)
            "waldo_wif_fuse_bwd": 4 * (m * 4 * hwd + m * 4 * hwd + 2 * u * 3 * hwd + m * 5 * hwd),
        }
