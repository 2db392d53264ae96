"""The warp-path part of one LVD training step at the reference's recipe -- the one place where the
reference differentiates THROUGH the path (models/synthesizer.py:815-841, scripts/cityscapes/train_lvd.sh:
128 x 256 with no full-resolution raster, 16 objects, 5-frame clips, ``ctx_mode "prev"``, ``include_self``,
layout filtering with weighted classes):

    decoder tail -> pose heads' affine -> estimate_alpha_grid_occ (TPS grids + grid inversion, compute_occ)
    -> decode_output (grid_to_flow + input_to_output) -> loss -> backward

with the tensors the networks outside the path would hand over as seeded leaves (decoder logits, pose head
outputs, occlusion scores, class logits).  ``bench.py --config LVD`` times it.

``objective="stand-in"`` (the default) closes the step with a plain quadratic of the outputs;
``objective="recipe"`` with the recipe's own four terms (``--s_vid_object_extractor_losses "ent_flt_edge" "l1_flow"
"cell_dis" "reg_mov"``, train_lvd.sh:15) on a seeded real flow: the moving-object target is built on the device at
every call, as the reference builds it at every step (``waldo_amd.supervision``).

``nets="reference"`` feeds the step from a seeded ``nets.LVD`` at the recipe's widths -- encoder, layer estimator, pose
estimator and object decoder in front of the same warp path (synthesizer.py:815-823) -- instead of from leaves: the
gradients then land in the networks' parameters.  ``nets="stand-in"`` (the default) is the step described above.
With ``nets="reference"``, ``optimizer="adam"`` / ``"adamw"`` / an ``optim.Adam`` ends the step as the reference does
(synthesizer.py:1057-1072) with ``optimizer.step(loss)`` on the device (``waldo_amd.optim``); None stops at the gradients.
"""
import types

import torch

from .. import functional as WF
from .. import optim, supervision
from ..nets import LVD, Warper, decode_output, estimate_alpha_grid_occ, flp
from ..nets.lvd import decoder_tail
from .utils import get_grid


def lvd_opt(**over):
    d = dict(latent_shape=[8, 16], obj_shape=[4, 4], time_dropout=0.0, num_obj=16, patch_size=16, scale_factor=1,
             dim=128, aspect_ratio=2, load_dim=0, num_perm_grid=1, normalize_alpha=False, use_lyt_filtering=True,
             use_lyt_opacity=True, weight_cls=True, min_cls=0.1, include_self=True, no_filter=False, allow_ghost=False)
    d.update(over)
    return types.SimpleNamespace(**d)


# the recipe's options of the moving-object target (scripts/cityscapes/train_lvd.sh:28-35; the Cityscapes channel lists
# of tools/options.py:628-630) and the weights of its four terms (train_lvd.sh:29-31; ent_flt_edge at the default of
# --s_lambda_ent_flt_edge, tools/options.py:461)
RECIPE_TARGET = dict(fg_idx=[0, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17, 18, 19], bg_idx=[1, 2, 3, 10, 11], other_idx=[9],
                     flow_thresh=0.02, mov_obj_thresh=0.005, blur_sigma=2.0, edge_size=15, reg_bg_mul=0.25, use_fg=True,
                     use_dominant_flow_other=True)
RECIPE_WEIGHTS = {"cell_dis": 10.0, "l1_flow": 1000.0, "reg_mov": 10.0, "ent_flt_edge": 1.0}
OBJECTIVES = ("stand-in", "recipe")
NETS = ("stand-in", "reference")


def recipe_net_opt(**over):
    """``nets.lvd_net_opt`` at scripts/cityscapes/train_lvd.sh: what ``lvd_opt`` holds for the warp path plus the
    networks' widths and switches (512 wide, 8 heads, two blocks each, layout + flow input)."""
    from ..nets.lvd import lvd_net_opt
    d = dict(vars(lvd_opt()), time_dropout=False, embed_dim=512, num_heads=8, oe_depth=2, pe_depth=2, oe_num_timesteps=5,
             num_lyt=LvdStep.num_lyt, input_rgb=False, input_lyt=True, input_flow=True, ctx_len=4, bound_rest=True,
             soft_bound_rest=True, pe_decoder_init_mode="five", pe_estimator_init_mode="", has_bg=True, pad_obj_alpha=3,
             pad_bg_alpha=3, init_scale_obj=0.25, mul_scale_obj=0.25, mul_delta_obj=0.2, circle_translate_bias=True,
             circle_translate_radius=0.2, pred_cls=True, bg_mul=1.2)
    d.update(over)
    return lvd_net_opt(**d)


class LvdStep:
    """``clips`` clips of 5 frames resident on ``device``; ``__call__`` runs forward, loss and backward once and
    returns the loss (the leaves' ``.grad`` hold the gradients).  ``optimizer`` (with ``nets="reference"``): None, "adam",
    "adamw" or an ``optim.Adam`` over the networks' parameters; the step then ends in ``optimizer.step(loss)``, and
    ``step.optimizer`` is it.  ``act_dtype`` (with ``nets="reference"``): the networks' ``act_dtype`` -- torch.bfloat16
    or torch.float16: they run under autocast with the 16-bit attention kernel, the warp path stays fp32.  The
    attention's backward is then the framework's recompute; ``with WF.token_attention_16bit_backward_route("kernel"):``
    around the call makes it the 16-bit backward kernel (``waldo_token_attention_bwd_dt``)."""

    frames, num_lyt = 5, 20

    def __init__(self, clips, device, seed=0, objective="stand-in", nets="stand-in", optimizer=None, act_dtype=None):
        if act_dtype is not None and nets != "reference":
            raise ValueError("LvdStep: act_dtype needs nets='reference' (the stand-in step has no networks)")
        if objective not in OBJECTIVES:
            raise ValueError(f"LvdStep: objective must be one of {OBJECTIVES}, got {objective!r}")
        if nets not in NETS:
            raise ValueError(f"LvdStep: nets must be one of {NETS}, got {nets!r}")
        if optimizer is not None and nets != "reference":
            raise ValueError("LvdStep: optimizer= needs nets='reference' (the stand-in step has leaves, no parameters)")
        self.objective = objective
        self.nets = nets
        self.optimizer = None
        self.net = None
        self.opt = o = lvd_opt()
        self.clips = b = clips
        t, no, nl = self.frames, o.num_obj, self.num_lyt
        lo, lb = o.obj_shape[0] * o.obj_shape[1], o.latent_shape[0] * o.latent_shape[1]
        h, w = o.dim, int(o.dim * o.aspect_ratio)
        ho = o.obj_shape[0] * o.patch_size
        self.warper = Warper(o).to(device)
        g = torch.Generator(device=device).manual_seed(seed)
        self.raw = torch.randn(b * no, 1, ho, ho, generator=g, device=device, requires_grad=True)
        self.pose_o = (0.3 * torch.randn(b * t, no, 6 + 2 * lo, generator=g, device=device)).requires_grad_()
        self.pose_b = (0.05 * torch.randn(b * t, 1, 6 + 2 * lb, generator=g, device=device)).requires_grad_()
        self.score = torch.randn(b, t, no, generator=g, device=device, requires_grad=True)
        self.cls_logit = torch.randn(b, no, nl, generator=g, device=device, requires_grad=True)
        self.inp = torch.randn(b, t, 3 + nl, h, w, generator=g, device=device)
        self.base_o = get_grid(*o.obj_shape).view(1, 1, lo, 2).to(device)
        self.base_b = get_grid(*o.latent_shape).view(1, 1, lb, 2).to(device)
        self.mul6 = torch.tensor([[[0.25, 0.25, 0.25, 0.25, 1.0, 1.0]]], device=device)
        self.bias_o = torch.tensor([[[0.25, 0.0, 0.0, 0.5, 0.0, 0.0]]], device=device)
        self.bias_b = torch.tensor([[[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]], device=device)
        self.bg_alpha = torch.ones(1, 1, h, w, device=device)
        # ctx_mode "prev" (synthesizer.py:833-835): every frame is predicted from the one before it
        self.ctx_ts = torch.roll(torch.arange(t, device=device), 1).view(1, 1, t).expand(b, -1, -1).contiguous()
        # (every frame is predicted, in order: an index MARKED as 0 .. T-1 lets time_gather hand out the clip itself)
        self.pred_ts = WF.arange_index(t, device)
        # (drawn after everything else: the leaves above are the same values with either objective)
        self.real_flow = (0.05 * torch.randn(b, t, 2, h, w, generator=g, device=device)) if objective == "recipe" else None
        self.leaves = [self.raw, self.pose_o, self.pose_b, self.score, self.cls_logit]
        self.shape = (b, t, no, lo, lb, ho)
        if nets == "reference":
            # (built last, from a generator state of its own: everything above keeps the stand-in step's values)
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                self.net = LVD(recipe_net_opt()).to(device)
            self.net.act_dtype = act_dtype
            if self.real_flow is None:
                self.real_flow = 0.05 * torch.randn(b, t, 2, h, w, generator=g, device=device)
            self.leaves = list(self.net.parameters())
            self.optimizer = optim.resolve(optimizer, self.leaves, "LvdStep")

    def _network_step(self):
        """The forward of synthesizer.py:810-841 through the networks; returns decode_output's tuple and obj_pose."""
        net, ctx_len = self.net, self.net.pose_estimator.ctx_len
        x = net(input=torch.cat([self.inp[:, :, 3:], self.real_flow], dim=2), mode="encode_input")
        x_obj, x_bg, cls = net(x=x[:, :ctx_len], mode="estimate_layer")
        obj_pose, bg_pose, occ_score = net(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")[:3]
        occ, oa, ba, grid = net(x_obj=x_obj, obj_pose=obj_pose, bg_pose=bg_pose, occ_score=occ_score,
                                mode="estimate_alpha_grid_occ")
        out = net(input=self.inp, grid=grid, occ=occ, obj_alpha=oa, bg_alpha=ba, ctx_ts=self.ctx_ts, pred_ts=self.pred_ts,
                  cls=cls, mode="decode_output")
        return out, obj_pose

    def __call__(self):
        b, t, no, lo, lb, ho = self.shape
        for x in self.leaves:
            x.grad = None
        if self.net is not None:
            out, obj_pose = self._network_step()
            return self._close(out, obj_pose)
        obj_alpha = decoder_tail(self.raw, init_bias=5.0).view(b, no, 1, ho, ho)
        obj_pose = flp.obj_pose_to_points(torch.tanh(self.pose_o), self.base_o, self.mul6, self.bias_o, 0.2)
        bg_pose = flp.bg_pose_to_points(torch.tanh(self.pose_b), self.base_b, self.bias_b, 1.2)
        occ, oa, ba, grid = estimate_alpha_grid_occ(self.warper, obj_alpha, self.bg_alpha,
                                                    obj_pose.view(b, t, no, lo, 2), bg_pose.view(b, t, 1, lb, 2),
                                                    self.score)
        out = decode_output(self.warper, self.inp, grid, occ, oa, ba, self.cls_logit.softmax(-1), self.ctx_ts,
                            self.pred_ts, restrict_to_ctx=False)
        return self._close(out, obj_pose)

    def _close(self, out, obj_pose):
        b, t, no, lo, lb, ho = self.shape
        if self.objective == "recipe":
            real_lyt = self.inp[:, :, 3:]
            target = supervision.moving_object_target(self.real_flow, real_lyt, **RECIPE_TARGET)
            # ctx_mode "prev" (synthesizer.py:849): the flow from the previous frame, for every frame but the first
            self.terms = supervision.recipe_terms(out[3], out[1][:, 0, 1:], self.real_flow, real_lyt,
                                                  obj_pose.view(b, t, no, lo, 2), self.opt.obj_shape, target)
            loss = sum(RECIPE_WEIGHTS[k] * v for k, v in self.terms.items())
        else:
            loss = out[0].square().mean() + out[1].square().mean() + out[3].mean()
        loss.backward()
        if self.optimizer is not None:
            self.optimizer.step(loss.detach())
        return loss

    def grads_finite(self):
        return all(bool(torch.isfinite(x.grad).all()) for x in self.leaves)
