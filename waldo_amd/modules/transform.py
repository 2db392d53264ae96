"""Drop-ins for the transformer modules of the reference's LVD and FLP networks (models/modules/transform.py):
``CustomNorm``, ``Mlp``, ``FullAttention``, ``CrossAttention``, ``ObjAttention``, ``ClsAttention``, ``CustomAttention``,
``Block`` and ``MultiBlocks`` -- the same constructor keywords, forward semantics and parameter names
(``multi_blocks.{i}.norm1.norm.weight``, ``.attn.attn.qkv.weight``, ``.attn.attn.q|kv|proj.*``, ``.mlp.fc1|fc2.*``,
``.attn.attn.noise_strength``), so that a reference checkpoint loads with ``strict=True``.

The Linear and LayerNorm layers stay the framework's (hipBLASLt).  The attention between them -- the reference's
matmul -> scale -> softmax -> matmul with the permutes of the packed projections, the ``cat`` of ObjAttention's two key
sets and the transpose in front of ``proj`` -- is one hand-written kernel, ``WF.token_attention``, which reads the
slices of ``qkv`` / ``kv`` where they lie.  ``fused = False`` (an attribute of every attention module; ``MultiBlocks``
and ``Block`` pass an assignment on) runs the reference's sequence of framework ops instead, and is the route on the CPU.
Under autocast the slices are 16-bit and take the framework route too, unless the caller has set
``WF.token_attention_16bit_route("kernel")`` -- as the networks' ``act_dtype`` does (nets/lvd.py ``_Net``) -- which
serves them with the 16-bit forward kernels.  Their backward is the framework's recompute unless the training code has
also set ``WF.token_attention_16bit_backward_route("kernel")`` around the step: the dense attention then differentiates
by ``waldo_token_attention_bwd_dt`` (the per-clip form below keeps the recompute).

With ``ctx_mask`` -- the future layer predictor's clips, of which a (B, T) mask selects the frames -- the tokens stay
PACKED, (B', N, C) over the selected frames as the reference's ``to_ctx`` leaves them, and the attention is
``WF.token_attention_clips`` on the slices of ``qkv`` / ``q`` / ``kv`` where they lie: within a clip the selected
query frames attend to the selected key frames.  That is what the reference's ``from_ctx`` -> dense (B, T N) attention
under a -inf mask -> ``to_ctx`` computes (transform.py:107-120, 146-156), without the dense tensors and without the
host read each of those three makes.  ``ctx_mask`` is a boolean tensor, as in the reference (one host read per call, to
size the packed tensors), or a ``ClipPlan``, which holds what the mask says as gather indices and offset tables;
``ClipPlan.first_frames`` builds one from integers alone, and a forward under such a plan reads nothing on the host.

What only the future predictor uses -- the block types ``cross`` and ``cls``, ``noise=True`` and ``ctx_mask`` -- is
served to a caller that asks for it with the keyword ``flp=True`` (``Block`` / ``MultiBlocks`` / ``CustomAttention`` /
``FullAttention``; ``nets.flp`` passes it).  Without it the modules are the LVD networks' as they were: those four are
refused.  ``CrossAttention`` and ``ClsAttention`` built directly need no keyword.

Not served, and refused in the constructor: spectral normalisation and the block types that neither the LVD nor the FLP
networks use (ctx, block_causal, skip, skip2)."""
import torch
import torch.nn as nn

from .. import functional as WF

_UNUSED_BLOCK_TYPES = ("ctx", "block_causal", "skip", "skip2")
_FLP_BLOCK_TYPES = {"cross": "CrossAttention", "cls": "ClsAttention"}


class ClipPlan:
    """A (B, T) frame mask as the packed tensors need it, for frames of ``tokens`` tokens each: ``index`` the flat
    (b T + t) ids of the selected frames in order and ``rest`` those of the others (int64: the gathers of ``to_ctx``
    and the scatters of ``from_ctx``), ``offsets`` / ``rest_offsets`` the int32 (B + 1,) tables of the clips' packed ROWS
    (``WF.token_attention_clips``), ``max_len`` / ``rest_max_len`` host integers no clip's rows exceed, ``frames`` /
    ``rest_frames`` the host counts.  ``mask`` is the boolean tensor itself."""

    def __init__(self, mask, tokens, index, rest, offsets, rest_offsets, max_len, rest_max_len, first=None):
        self.mask, self.tokens = mask, int(tokens)
        self.first = first  # built from integers: the number of leading frames selected in every clip
        self.batch, self.steps = mask.shape
        self.index, self.rest, self.offsets, self.rest_offsets = index, rest, offsets, rest_offsets
        self.max_len, self.rest_max_len = int(max_len), int(rest_max_len)
        self.frames, self.rest_frames = index.numel(), rest.numel()

    @staticmethod
    def _of(mask, tokens, frames):
        """From a mask whose number of selected frames is known on the host: a stable sort and two cumsums."""
        flat = mask.reshape(-1)
        order = torch.argsort((~flat).to(torch.uint8), stable=True)
        full = mask.shape[1] * int(tokens)
        return ClipPlan(mask, tokens, order[:frames], order[frames:], WF.clip_offsets(mask, tokens),
                        WF.clip_offsets(~mask, tokens), full, full)

    @staticmethod
    def from_mask(mask, tokens):
        """From a boolean (B, T) tensor: ONE host read, the number of selected frames."""
        if mask.dim() != 2 or mask.dtype != torch.bool:
            raise ValueError(f"ClipPlan: ctx_mask must be a boolean (B, T) tensor, got {mask.dtype} {tuple(mask.shape)}")
        return ClipPlan._of(mask, tokens, int(mask.sum()))

    @staticmethod
    def first_frames(batch, steps, ctx_len, tokens, device=None):
        """The first ``ctx_len`` frames of every clip, from integers alone: no device read at all."""
        if not 0 <= ctx_len <= steps:
            raise ValueError(f"ClipPlan.first_frames: 0 <= ctx_len <= steps, got ctx_len={ctx_len} steps={steps}")
        t = torch.arange(steps, device=device)
        ids = torch.arange(batch, device=device)[:, None] * steps + t[None, :]
        off = torch.arange(batch + 1, device=device, dtype=torch.int32)
        return ClipPlan((t < ctx_len).expand(batch, steps), tokens, ids[:, :ctx_len].reshape(-1),
                        ids[:, ctx_len:].reshape(-1), off * (ctx_len * tokens), off * ((steps - ctx_len) * tokens),
                        ctx_len * tokens, (steps - ctx_len) * tokens, first=ctx_len)

    def padded(self):
        """The plan of this mask with one selected frame in front of every clip (FLP's ``cat_z``); no host read."""
        if self.first is not None:
            return ClipPlan.first_frames(self.batch, self.steps + 1, self.first + 1, self.tokens, self.mask.device)
        mask = torch.cat([torch.ones_like(self.mask[:, :1]), self.mask], dim=1)
        return ClipPlan._of(mask, self.tokens, self.frames + self.batch)

    def complement(self):
        """The plan of ``~mask``: the same tensors with the two sides exchanged."""
        return ClipPlan(~self.mask, self.tokens, self.rest, self.index, self.rest_offsets, self.offsets,
                        self.rest_max_len, self.max_len)

    @staticmethod
    def of(ctx_mask, tokens):
        """``ctx_mask`` as a plan: a ``ClipPlan`` as it is (its frames must have ``tokens`` tokens), a tensor through
        ``from_mask``."""
        if isinstance(ctx_mask, ClipPlan):
            if ctx_mask.tokens != tokens:
                raise ValueError(f"ClipPlan: built for frames of {ctx_mask.tokens} tokens, the input has {tokens}")
            return ctx_mask
        return ClipPlan.from_mask(ctx_mask, tokens)


def _plain_linear(spectral_norm_layer, what):
    if spectral_norm_layer is not None:
        raise NotImplementedError(f"{what}: spectral_norm_layer={spectral_norm_layer!r} (the LVD networks use None)")


class PixelNorm(nn.Module):
    def forward(self, input):
        return input * torch.rsqrt(torch.mean(input ** 2, dim=2, keepdim=True) + 1e-8)


class CustomNorm(nn.Module):
    """The norms of token tensors (B, N, C): ``ln`` (LayerNorm), ``ln_not_affine`` and ``pn`` (PixelNorm: over the
    channels of every token).  The norm lives under ``.norm``, as in the reference's state dict.  (The norms of image
    planes, ``ln2d`` / ``bn2d``, are ``modules.conv.CustomNorm``.)"""

    def __init__(self, norm_layer, dim):
        super().__init__()
        self.norm_type = norm_layer
        if norm_layer == "ln":
            self.norm = nn.LayerNorm(dim)
        elif norm_layer == "ln_not_affine":
            self.norm = nn.LayerNorm(dim, elementwise_affine=False)
        elif norm_layer == "pn":
            self.norm = PixelNorm()
        else:
            raise ValueError(f"CustomNorm: norm_layer must be 'ln', 'ln_not_affine' or 'pn', got {norm_layer!r}")

    def forward(self, x):
        return self.norm(x)


class Mlp(nn.Module):
    def __init__(self, dim, spectral_norm_layer, mul=4, out_dim=None):
        super().__init__()
        _plain_linear(spectral_norm_layer, "Mlp")
        self.fc1 = nn.Linear(dim, mul * dim)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(mul * dim, dim if out_dim is None else out_dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _Attention(nn.Module):
    """What the two attentions share: the head split and the route switch."""

    def __init__(self, dim, num_heads, spectral_norm_layer, what):
        super().__init__()
        _plain_linear(spectral_norm_layer, what)
        if dim % num_heads:
            raise ValueError(f"{what}: dim={dim} is not a multiple of num_heads={num_heads}")
        self.dim = dim
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.fused = True  # False: the reference's sequence of framework ops

    def _attend(self, q, k, v, k2=None, v2=None):
        op = WF.token_attention if self.fused else WF.token_attention_framework
        return op(q, k, v, k2, v2, scale=self.scale)

    def _heads(self, x, b, parts):
        """A packed projection (B', N', parts C) as ``parts`` views (b, N, H, D) -- slices, no copies."""
        x = x.reshape(b, -1, parts, self.num_heads, self.dim // self.num_heads)
        return x.unbind(2) if parts > 1 else (x[:, :, 0],)

    def _rows(self, x, parts, frames, what):
        """A projection (B', N, parts C) of packed frames as ``parts`` views (B' N, H, D) -- slices, no copies."""
        if x.shape[0] != frames:
            raise ValueError(f"{what}: {x.shape[0]} packed frames, ctx_mask selects {frames}")
        x = x.reshape(-1, parts, self.num_heads, self.dim // self.num_heads)
        return x.unbind(1) if parts > 1 else (x[:, 0],)

    def _attend_clips(self, q, k, v, q_offsets, k_offsets, max_q_len, max_k_len):
        op = WF.token_attention_clips if self.fused else WF.token_attention_clips_framework
        return op(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len, scale=self.scale)

    def _init_noise(self, noise):
        self.noise = noise
        if noise:
            self.noise_strength = nn.Parameter(torch.zeros([]))

    def _noisy(self, x):
        if not self.noise:
            return x
        return x + torch.randn([x.size(0), x.size(1), 1], device=x.device, dtype=x.dtype) * self.noise_strength


class FullAttention(_Attention):
    """Self-attention over the tokens of x (B, N, C): models/modules/transform.py:87-122.  With ``ctx_mask`` x is
    (B', N, C), the selected frames packed, and every clip's selected frames attend to one another.  ``noise`` and
    ``ctx_mask`` are the future predictor's: served with ``flp=True``."""

    def __init__(self, dim, num_heads, spectral_norm_layer, noise, flp=False, **kwargs):
        super().__init__(dim, num_heads, spectral_norm_layer, "FullAttention")
        if noise and not flp:
            raise NotImplementedError("FullAttention: noise=True is the future predictor's (the LVD networks use False): "
                                      "pass flp=True")
        self.flp = bool(flp)
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.proj = nn.Linear(dim, dim)
        self._init_noise(noise)

    def forward(self, x, ctx_mask=None, **kwargs):
        if ctx_mask is not None and not self.flp:
            raise NotImplementedError("FullAttention: ctx_mask is the future predictor's masked clips: build the module "
                                      "with flp=True")
        qkv = self.qkv(self._noisy(x))
        if ctx_mask is None:
            q, k, v = self._heads(qkv, x.shape[0], 3)
            return self.proj(self._attend(q, k, v))
        plan = ClipPlan.of(ctx_mask, x.shape[1])
        q, k, v = self._rows(qkv, 3, plan.frames, "FullAttention")
        out = self._attend_clips(q, k, v, plan.offsets, plan.offsets, plan.max_len, plan.max_len)
        return self.proj(out.view(x.shape))


class CrossAttention(_Attention):
    """The frames ``ctx_mask`` does NOT select, x_pred (B'', N, C) packed, attend to their clip's selected frames,
    x_ctx (B', N, C) packed: models/modules/transform.py:125-158."""

    def __init__(self, dim, num_heads, spectral_norm_layer, noise, **kwargs):
        super().__init__(dim, num_heads, spectral_norm_layer, "CrossAttention")
        self.q = nn.Linear(dim, dim, bias=False)
        self.kv = nn.Linear(dim, dim * 2, bias=False)
        self.proj = nn.Linear(dim, dim)
        self._init_noise(noise)

    def forward(self, x_pred, x_ctx, ctx_mask=None, **kwargs):
        if ctx_mask is None:
            raise ValueError("CrossAttention: ctx_mask is required")
        plan = ClipPlan.of(ctx_mask, x_pred.shape[1])
        q, = self._rows(self.q(self._noisy(x_pred)), 1, plan.rest_frames, "CrossAttention: x_pred")
        k, v = self._rows(self.kv(x_ctx), 2, plan.frames, "CrossAttention: x_ctx")
        out = self._attend_clips(q, k, v, plan.rest_offsets, plan.offsets, plan.rest_max_len, plan.max_len)
        return self.proj(out.view(x_pred.shape))


class ObjAttention(_Attention):
    """The object tokens x_obj (B, No Lo, C) attend to their own keys FOLLOWED BY those of the context x_ctx
    (B T, L, C), whose T frames are one key sequence per clip: models/modules/transform.py:161-187."""

    def __init__(self, dim, num_heads, spectral_norm_layer, **kwargs):
        super().__init__(dim, num_heads, spectral_norm_layer, "ObjAttention")
        self.q = nn.Linear(dim, dim, bias=False)
        self.kv = nn.Linear(dim, dim * 2, bias=False)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x_obj, x_ctx, **kwargs):
        b = x_obj.size(0)
        q, = self._heads(self.q(x_obj), b, 1)
        k_obj, v_obj = self._heads(self.kv(x_obj), b, 2)
        k, v = self._heads(self.kv(x_ctx), b, 2)
        return self.proj(self._attend(q, k_obj, v_obj, k, v))


class ClsAttention(_Attention):
    """One class token per sequence, z_cls (B, 1, C), attends to itself FOLLOWED BY the tokens x_ctx (B, N, C):
    models/modules/transform.py:190-211.  ``kv`` has no bias, so ``kv(cat[z_cls, x_ctx])`` is the two key segments of
    ``WF.token_attention`` with one query."""

    def __init__(self, dim, num_heads, spectral_norm_layer, **kwargs):
        super().__init__(dim, num_heads, spectral_norm_layer, "ClsAttention")
        self.q = nn.Linear(dim, dim, bias=False)
        self.kv = nn.Linear(dim, dim * 2, bias=False)
        self.proj = nn.Linear(dim, dim)

    def forward(self, z_cls, x_ctx, **kwargs):
        b = z_cls.size(0)
        q, = self._heads(self.q(z_cls), b, 1)
        k_cls, v_cls = self._heads(self.kv(z_cls), b, 2)
        k, v = self._heads(self.kv(x_ctx), b, 2)
        return self.proj(self._attend(q, k_cls, v_cls, k, v))


class CustomAttention(nn.Module):
    def __init__(self, block_type, **kwargs):
        super().__init__()
        if block_type in _FLP_BLOCK_TYPES and not kwargs.get("flp", False):
            raise NotImplementedError(f"CustomAttention: block_type={block_type!r} belongs to the future predictor: pass "
                                      f"flp=True (or build {_FLP_BLOCK_TYPES[block_type]} itself)")
        if block_type in ("full", "full_with_cond_norm"):
            self.attn = FullAttention(**kwargs)
        elif block_type == "cross":
            self.attn = CrossAttention(**kwargs)
        elif block_type == "obj":
            self.attn = ObjAttention(**kwargs)
        elif block_type == "cls":
            self.attn = ClsAttention(**kwargs)
        elif block_type in _UNUSED_BLOCK_TYPES:
            raise NotImplementedError(f"CustomAttention: block_type={block_type!r} (neither the LVD nor the FLP networks "
                                      f"use it)")
        else:
            raise ValueError(f"CustomAttention: unknown block_type {block_type!r}")

    def forward(self, x, **kwargs):
        return self.attn(x, **kwargs)


class _Identity:  # (not a module: the reference's blocks without dropout have no dp1 / dp2 entries either)
    def __call__(self, x):
        return x


class Block(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        dim, norm_layer = kwargs["dim"], kwargs["norm_layer"]
        spectral_norm_layer, block_type = kwargs["spectral_norm_layer"], kwargs["block_type"]
        self.cond_norm = block_type == "full_with_cond_norm"
        if self.cond_norm:
            if norm_layer == "ln":
                raise ValueError("Block: full_with_cond_norm needs a norm without an affine of its own")
            self.ab = Mlp(dim, spectral_norm_layer, out_dim=4 * dim)
        self.norm1 = CustomNorm(norm_layer, dim)
        self.attn = CustomAttention(**kwargs)
        self.norm2 = CustomNorm(norm_layer, dim)
        self.mlp = Mlp(dim, spectral_norm_layer)
        self.block_type = block_type
        if kwargs.get("dropout", 0) > 0:
            self.dp1, self.dp2 = nn.Dropout(kwargs["dropout"]), nn.Dropout(kwargs["dropout"])
        else:
            self.dp1 = self.dp2 = _Identity()

    @property
    def fused(self):
        return self.attn.attn.fused

    @fused.setter
    def fused(self, value):
        self.attn.attn.fused = bool(value)

    def _modulation(self, x, kwargs):
        """(scale, shift) in front of the attention and in front of the MLP: from ``z_cond`` with
        ``full_with_cond_norm``, else the identity."""
        if not self.cond_norm:
            return (1., 0.), (1., 0.)
        a1, b1, a2, b2 = self.ab(kwargs["z_cond"]).view(x.size(0), 1, 4, -1).unbind(2)
        return (a1, b1), (a2, b2)

    def forward(self, x, **kwargs):
        """Pre-norm residual block: x + attn(mod(norm1 x)), then + mlp(mod(norm2 .))."""
        branches = ((self.norm1, lambda y: self.attn(y, **kwargs), self.dp1), (self.norm2, self.mlp, self.dp2))
        for (norm, branch, drop), (scale, shift) in zip(branches, self._modulation(x, kwargs)):
            x = x + drop(branch(scale * norm(x) + shift))
        return x


class MultiBlocks(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        self.multi_blocks = nn.ModuleList([Block(**kwargs) for _ in range(kwargs["depth"])])

    @property
    def fused(self):
        return all(block.fused for block in self.multi_blocks)

    @fused.setter
    def fused(self, value):
        for block in self.multi_blocks:
            block.fused = value

    def forward(self, z, **kwargs):
        for block in self.multi_blocks:
            z = block(z, **kwargs)
        return z
