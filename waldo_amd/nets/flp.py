"""Host-side mirror of the one step of the reference's models/nets/flp.py that feeds the path: the
pose heads' affine (flp.py:259-273; the same arithmetic sits in the LVD pose estimator,
models/nets/lvd.py:440-449).  The transformer that predicts the poses is outside this path; what
it hands over -- (B', No, 6 + 2 Lo) object poses and (B', 1, 6 + 2 L) background poses, after
``tanh`` and the optional ``+ last`` -- becomes the TPS control points ``Warper.forward`` consumes,
in one kernel forward and one backward (csrc/producers.hip) instead of seven framework launches.

Below them, the networks themselves: ``FLP`` and its parts as drop-ins.
"""
import torch
import torch.nn as nn

from .. import functional as WF
from ..modules.transform import ClipPlan
from ..tools.utils import get_grid
from .lvd import _Net


def obj_pose_to_points(pred_obj_pose, tgt_pts_obj, mul_obj, bias_obj, mul_delta_obj=1.0):
    """flp.py:260-265.  pred_obj_pose (B', No, 6 + 2 Lo); tgt_pts_obj (1, 1, Lo, 2); mul_obj /
    bias_obj (1, 1, 6) buffers (bias_obj may be the scalar 0 of the `no_bias` option, flp.py:208).
    Returns the object control points (B', No, Lo, 2)."""
    bias = bias_obj if hasattr(bias_obj, "reshape") else mul_obj.new_full((6,), float(bias_obj))
    return WF.pose_affine(pred_obj_pose, mul_obj, bias, tgt_pts_obj, mul_delta=mul_delta_obj, pts_mul=1.0)


def bg_pose_to_points(pred_bg_pose, tgt_pts_bg, bias_bg, bg_mul=1.0):
    """flp.py:268-273.  pred_bg_pose (B', 1, 6 + 2 L); tgt_pts_bg (1, 1, L, 2); bias_bg (1, 1, 6) or
    the scalar 0.  Returns the background control points (B', 1, L, 2)."""
    ones = tgt_pts_bg.new_ones(6)
    bias = bias_bg if hasattr(bias_bg, "reshape") else ones * float(bias_bg)
    return WF.pose_affine(pred_bg_pose, ones, bias, tgt_pts_bg, mul_delta=1.0, pts_mul=bg_mul)


# --------------------------------------------------------------------------------------
# Drop-ins for the reference's future layer predictor (models/nets/flp.py): FLP, LatentCompressor, PoseEncoder and
# PoseDecoder -- the same constructors (from ``opt``), forward signatures, parameter AND buffer names, so that a reference
# ``pg`` checkpoint loads with ``strict=True``.  The tokens of the frames a (B, T) ``ctx_mask`` selects stay PACKED from
# the embedding to the heads: the blocks' attention is ``WF.token_attention_clips`` over per-clip segments of the packed
# rows (modules/transform.py), where the reference scatters to a dense (B, T N) tensor, masks and gathers back with a
# host read each.  ``ctx_mask`` is a boolean tensor (one host read per forward) or a ``FlpPlan``; with
# ``FlpPlan.first_frames`` a forward reads nothing on the host and can be captured in a graph.  The pose tail is
# ``obj_pose_to_points`` / ``bg_pose_to_points`` above.  ``fused = False``: framework ops only (the CPU route).
# --------------------------------------------------------------------------------------
def flp_net_opt(**over):
    """The reference's defaults (tools/options.py) for every field its models/nets/flp.py reads; ``over`` overrides."""
    import types
    d = dict(latent_shape=[4, 8], obj_shape=[4, 4], embed_dim=512, num_heads=8, norm_layer="ln", dropout=0, num_obj=1,
             aspect_ratio=1.0, vid_len=16, ctx_len=10, init_scale_obj=1., mul_scale_obj=1., mul_delta_obj=1.,
             pg_com_depth=2, pg_enc_depth=4, pg_dec_depth=4, pg_num_timesteps=5, pg_embed_noise=False,
             pg_inject_noise=False, pg_modulate_noise=False, cat_z=True, use_last_pose_decoder=False,
             unconstrained_pose_decoder=False, bg_mul_pose_decoder=1., zero_init_dec=True)
    unknown = set(over) - set(d)
    if unknown:
        raise TypeError(f"flp_net_opt: unknown fields {sorted(unknown)}")
    d.update(over)
    return types.SimpleNamespace(**d)


class FlpPlan:
    """What FLP needs of a (B, T) ``ctx_mask`` for layer frames of ``tokens`` = No + 1 tokens: ``frames`` the
    ``ClipPlan`` of the mask itself (the gathers of the poses, the scatter of the predictions) and ``blocks`` that of
    the mask the blocks see -- with ``cat_z`` one selected frame, the compressed latents, in front of every clip."""

    def __init__(self, frames, cat_z):
        self.frames, self.cat_z = frames, bool(cat_z)
        self.blocks = frames.padded() if cat_z else frames
        self.pred_blocks = self.blocks.complement()
        # the clip of every predicted frame (use_last_pose_decoder)
        self.rest_clip = torch.div(self.blocks.rest, self.blocks.steps, rounding_mode="floor")

    @staticmethod
    def from_mask(ctx_mask, tokens, cat_z=True):
        """From a boolean (B, T) tensor: one host read."""
        return FlpPlan(ClipPlan.from_mask(ctx_mask, tokens), cat_z)

    @staticmethod
    def first_frames(batch, steps, ctx_len, tokens, cat_z=True, device=None):
        """The first ``ctx_len`` of ``steps`` frames of every clip, from integers alone: no device read."""
        return FlpPlan(ClipPlan.first_frames(batch, steps, ctx_len, tokens, device), cat_z)

    @staticmethod
    def of(ctx_mask, tokens, cat_z):
        if isinstance(ctx_mask, FlpPlan):
            if ctx_mask.cat_z != bool(cat_z) or ctx_mask.frames.tokens != tokens:
                raise ValueError(f"FlpPlan: built for cat_z={ctx_mask.cat_z} and {ctx_mask.frames.tokens} tokens per "
                                 f"frame, the network has cat_z={bool(cat_z)} and {tokens}")
            return ctx_mask
        return FlpPlan.from_mask(ctx_mask, tokens, cat_z)


def _select(x, index):
    """``to_ctx``: the frames ``index`` of x (B, T, ...) -> (B', ...)."""
    return x.flatten(0, 1).index_select(0, index)


def _block_args(opt, block_type, depth, norm_layer=None, noise=False, dropout=True):
    args = dict(block_type=block_type, depth=depth, dim=opt.embed_dim, num_heads=opt.num_heads,
                norm_layer=opt.norm_layer if norm_layer is None else norm_layer, spectral_norm_layer=None, noise=noise,
                flp=True)   # (cross, cls, noise and ctx_mask: modules/transform.py serves them on request)
    if dropout:
        args["dropout"] = opt.dropout
    return args


class LatentCompressor(_Net):
    """flp.py:288-314: a class token per layer attends to the layer's tokens (``cls`` blocks)."""

    def __init__(self, opt, depth, spectral_norm_layer=None):
        from ..modules.conv import init_weights
        from ..modules.transform import CustomNorm, MultiBlocks
        super().__init__()
        self.cls_embed = nn.Parameter(torch.randn(1, 1, opt.embed_dim))
        args = _block_args(opt, "cls", depth)
        args["spectral_norm_layer"] = spectral_norm_layer
        del args["noise"]
        self.norm = CustomNorm(opt.norm_layer, opt.embed_dim)
        self.blocks = MultiBlocks(**args)
        nn.init.trunc_normal_(self.cls_embed, std=.02)
        self.apply(init_weights)

    def forward(self, x):
        lead = x.shape[:2] if x.ndim == 4 else None
        if lead is not None:
            x = x.reshape(-1, *x.shape[2:])
        z_cls = self.blocks(self.cls_embed.expand(x.size(0), -1, -1), x_ctx=self.norm(x))
        return z_cls if lead is None or x.size(0) == 0 else z_cls.reshape(*lead, *z_cls.shape[1:])


class PoseEncoder(_Net):
    """flp.py:32-100: the context frames' poses as one token per layer, [compressed latents,] + time and layer
    embeddings, self-attention among each clip's context frames; the frames to predict leave as their embeddings."""

    def __init__(self, opt, depth, num_timesteps, embed_noise):
        from ..modules.conv import init_weights
        from ..modules.transform import CustomNorm, MultiBlocks
        super().__init__()
        self.latent_size = opt.latent_shape[0] * opt.latent_shape[1]
        self.latent_obj_size = opt.obj_shape[0] * opt.obj_shape[1]
        self.embed_noise = embed_noise
        self.cat_z = opt.cat_z
        self.lay_embed = nn.Parameter(torch.randn(1, 1, opt.num_obj + 1, opt.embed_dim))
        self.time_embed = nn.Parameter(torch.randn(1, num_timesteps + 1, 1, opt.embed_dim))
        self.to_obj_emb = nn.Linear(self.latent_obj_size * 2 + 1, opt.embed_dim)
        self.to_bg_emb = nn.Linear(self.latent_size * 2, opt.embed_dim)
        self.blocks = MultiBlocks(**_block_args(opt, "full", depth))
        self.norm = CustomNorm(opt.norm_layer, opt.embed_dim)
        nn.init.trunc_normal_(self.lay_embed, std=.02)
        nn.init.trunc_normal_(self.time_embed, std=.02)
        self.apply(init_weights)

    def forward(self, obj_pose, bg_pose, occ_score, z, ctx_mask):
        c, l = z.size(-1), self.latent_size
        b, t, no, lo, _ = obj_pose.shape
        plan = FlpPlan.of(ctx_mask, no + 1, self.cat_z)
        frames, blocks = plan.frames, plan.blocks
        # the context frames' tokens (B', No + 1, C), the background's first
        obj = torch.cat([_select(obj_pose, frames.index).reshape(-1, no, lo * 2),
                         _select(occ_score, frames.index).reshape(-1, no, 1)], dim=2)
        x = torch.cat([self.to_bg_emb(_select(bg_pose, frames.index).reshape(-1, 1, l * 2)), self.to_obj_emb(obj)], dim=1)
        # the embeddings of every frame the blocks' mask covers (B, T', No + 1, C); the frames to predict leave as these
        if blocks.steps > self.time_embed.shape[1]:
            raise ValueError(f"PoseEncoder: {t} frames, the time embedding has {self.time_embed.shape[1] - self.cat_z}")
        embed = self.time_embed[:, :blocks.steps] + self.lay_embed
        if self.cat_z:
            # [z, context frames] of every clip: z is frame 0 of the T + 1, and the context frame b T + t of the packed
            # poses is frame b (T + 1) + t + 1 there; then the frames the blocks' mask selects, packed
            dense = x.new_zeros(b, t + 1, no + 1, c)
            dense[:, 0] = z.view(b, no + 1, c)
            at = frames.index + torch.div(frames.index, t, rounding_mode="floor") + 1
            dense = dense.flatten(0, 1).index_copy(0, at, x).view(b, t + 1, no + 1, c)
            x = _select(dense + embed, blocks.index)
        else:
            x = x + _select(embed.expand(b, -1, -1, -1), frames.index) + z.mean() * 0  # (as the reference: z stays used)
        x = self.norm(self.blocks(x, ctx_mask=blocks))
        x_init = embed.expand(b, -1, -1, -1)
        if self.embed_noise:
            x_init = x_init + torch.randn(b, 1, 1, c, device=x.device, dtype=x.dtype)
        out = x_init.flatten(0, 1).index_copy(0, blocks.index, x)
        return out.view(b, blocks.steps, no + 1, c)


class PoseDecoder(_Net):
    """flp.py:174-285: the frames to predict, packed, alternate self-attention among themselves and cross-attention to
    their clip's context frames; two linear heads and the pose affine turn their tokens into control points."""

    def __init__(self, opt, depth, inject_noise, modulate_noise):
        from ..modules.conv import init_weights
        from ..modules.transform import Block, CustomNorm
        super().__init__()
        self.latent_size = opt.latent_shape[0] * opt.latent_shape[1]
        self.latent_obj_size = opt.obj_shape[0] * opt.obj_shape[1]
        self.modulate_noise = modulate_noise
        self.embed_dim = opt.embed_dim
        self.num_obj = opt.num_obj
        self.use_last = opt.use_last_pose_decoder
        self.bg_mul = opt.bg_mul_pose_decoder
        self.cat_z = opt.cat_z
        args = _block_args(opt, "full_with_cond_norm" if modulate_noise else "full", depth,
                           "ln_not_affine" if modulate_noise else None, inject_noise, dropout=False)
        self.self_blocks = nn.ModuleList([Block(**args) for _ in range(depth)])
        args = _block_args(opt, "cross", depth, dropout=False)
        self.cross_blocks = nn.ModuleList([Block(**args) for _ in range(depth)])
        if opt.unconstrained_pose_decoder:
            mul_delta_obj, init_scale_obj, mul_scale_obj = 1, 1, 1
        else:
            mul_delta_obj, init_scale_obj, mul_scale_obj = opt.mul_delta_obj, opt.init_scale_obj, opt.mul_scale_obj
        self.mul_delta_obj = mul_delta_obj
        if opt.use_last_pose_decoder:
            self.bias_obj = 0
            self.bias_bg = 0
        else:
            self.register_buffer("bias_obj", torch.tensor([[[init_scale_obj, 0., 0., opt.aspect_ratio * init_scale_obj,
                                                             0., 0.]]]))
            self.register_buffer("bias_bg", torch.tensor([[[1., 0., 0., 1., 0., 0.]]]))
        self.register_buffer("tgt_pts_obj", get_grid(*opt.obj_shape).view(1, 1, self.latent_obj_size, 2))
        self.register_buffer("mul_obj", torch.tensor([[[mul_scale_obj, mul_scale_obj, mul_scale_obj, mul_scale_obj,
                                                        1., 1.]]]))
        self.register_buffer("tgt_pts_bg", get_grid(*opt.latent_shape).view(1, 1, self.latent_size, 2))
        self.norm = CustomNorm(opt.norm_layer, opt.embed_dim)
        self.obj_head = nn.Linear(opt.embed_dim, 6 + 2 * self.latent_obj_size + 1)
        self.bg_head = nn.Linear(opt.embed_dim, 6 + 2 * self.latent_size)
        self.apply(init_weights)
        if opt.zero_init_dec:
            for p in (self.obj_head.weight, self.obj_head.bias, self.bg_head.weight, self.bg_head.bias):
                p.data.zero_()

    def _points(self, obj, bg):
        """The pose affine (flp.py:259-273): the kernel on the GPU, the reference's arithmetic with ``fused = False``."""
        if self.fused and obj.is_cuda and obj.dtype == torch.float32:
            return (obj_pose_to_points(obj, self.tgt_pts_obj, self.mul_obj, self.bias_obj, self.mul_delta_obj),
                    bg_pose_to_points(bg, self.tgt_pts_bg, self.bias_bg, self.bg_mul))
        no, lo, l = self.num_obj, self.latent_obj_size, self.latent_size

        def through(pts, transform):
            return torch.cat([pts, torch.ones_like(pts[..., :1])], dim=-1) @ transform

        transform = (self.mul_obj * obj[:, :, :6] + self.bias_obj).view(-1, no, 3, 2)
        pts = self.tgt_pts_obj.expand(-1, no, -1, -1) + (self.mul_delta_obj * obj[:, :, 6:]).view(-1, no, lo, 2)
        bg_transform = (bg[:, :, :6] + self.bias_bg).view(-1, 1, 3, 2)
        bg_pts = self.bg_mul * self.tgt_pts_bg + bg[:, :, 6:].view(-1, 1, l, 2)
        return through(pts, transform), through(bg_pts, bg_transform)

    def forward(self, obj_pose, bg_pose, occ_score, x, ctx_mask, last_obj, last_bg, eps=1e-6):
        l, lo, no, c = self.latent_size, self.latent_obj_size, self.num_obj, self.embed_dim
        plan = FlpPlan.of(ctx_mask, no + 1, self.cat_z)
        blocks, pred = plan.blocks, plan.pred_blocks
        x_ctx, x_pred = _select(x, blocks.index), _select(x, blocks.rest)
        z_cond = torch.randn([x_pred.size(0), 1, c], device=x.device, dtype=x.dtype) if self.modulate_noise else None
        with self._act_region(x):
            for self_block, cross_block in zip(self.self_blocks, self.cross_blocks):
                x_pred = self_block(x_pred, ctx_mask=pred, z_cond=z_cond)
                x_pred = cross_block(x_pred, x_ctx=x_ctx, ctx_mask=blocks)
            x_pred = self.norm(x_pred)
            x_obj = self.obj_head(x_pred[:, 1:]).view(-1, no, 6 + 2 * lo + 1)
            x_bg = self.bg_head(x_pred[:, :1]).view(-1, 1, 6 + 2 * l)
        x_obj, x_bg = self._fp32(x_obj, x_bg)   # poses and occlusion scores: the warp path's
        pred_obj, pred_occ, pred_bg = x_obj[:, :, :-1].tanh(), x_obj[:, :, -1], x_bg.tanh()
        if self.use_last:
            pred_obj = pred_obj + last_obj.index_select(0, plan.rest_clip)
            pred_bg = pred_bg + last_bg.index_select(0, plan.rest_clip)
        pred_obj, pred_bg = self._points(pred_obj, pred_bg)
        # the context frames as they came in, the others predicted
        rest = plan.frames.rest
        fill = lambda full, part: full.flatten(0, 1).index_copy(0, rest, part.to(full.dtype)).view(full.shape)  # noqa: E731
        return fill(obj_pose, pred_obj), fill(bg_pose, pred_bg.view(-1, *bg_pose.shape[2:])), fill(occ_score, pred_occ)


class FLP(_Net):
    """flp.py:8-29.  ``ctx_mask``: a boolean (B, T) tensor, as in the reference, or a ``FlpPlan``.  ``act_dtype``
    (``_Net.act_dtype``): the compressor, the encoder and the decoder's blocks and heads under autocast with the 16-bit
    attention kernel; the predicted poses and occlusion scores leave in fp32."""

    def __init__(self, opt):
        super().__init__()
        self.compress = LatentCompressor(opt, opt.pg_com_depth)
        self.encode = PoseEncoder(opt, opt.pg_enc_depth, opt.pg_num_timesteps, opt.pg_embed_noise)
        self.decode = PoseDecoder(opt, opt.pg_dec_depth, opt.pg_inject_noise, opt.pg_modulate_noise)
        self.num_obj, self.cat_z = opt.num_obj, opt.cat_z

    def plan(self, batch, steps, ctx_len, device=None):
        """The ``FlpPlan`` of "the first ``ctx_len`` of ``steps`` frames of every clip", from integers alone."""
        return FlpPlan.first_frames(batch, steps, ctx_len, self.num_obj + 1, self.cat_z, device)

    def forward(self, obj_pose, bg_pose, occ_score, x_obj, x_bg, last_obj, last_bg, ctx_mask=None, mode="training"):
        if mode != "training":
            raise ValueError(f"FLP: mode must be 'training', got {mode!r}")
        if ctx_mask is None:
            raise ValueError("FLP: ctx_mask is required")
        plan = FlpPlan.of(ctx_mask, self.num_obj + 1, self.cat_z)
        with self._act_region(x_obj):
            z = torch.cat([self.compress(x_bg.unsqueeze(1)), self.compress(x_obj)], dim=1)
            x = self.encode(obj_pose, bg_pose, occ_score, z, plan)
        return self.decode(obj_pose, bg_pose, occ_score, x, plan, last_obj, last_bg)
