"""Drop-ins for the transformer modules of the reference's LVD networks (models/modules/transform.py): ``CustomNorm``,
``Mlp``, ``FullAttention``, ``ObjAttention``, ``CustomAttention``, ``Block`` and ``MultiBlocks`` -- the same constructor
keywords, forward semantics and parameter names (``multi_blocks.{i}.norm1.norm.weight``, ``.attn.attn.qkv.weight``,
``.attn.attn.q|kv|proj.*``, ``.mlp.fc1|fc2.*``), so that a reference checkpoint loads with ``strict=True``.

The Linear and LayerNorm layers stay the framework's (hipBLASLt).  The attention between them -- the reference's
matmul -> scale -> softmax -> matmul with the permutes of the packed projections, the ``cat`` of ObjAttention's two key
sets and the transpose in front of ``proj`` -- is one hand-written kernel, ``WF.token_attention``, which reads the
slices of ``qkv`` / ``kv`` where they lie.  ``fused = False`` (an attribute of every attention module; ``MultiBlocks``
and ``Block`` pass an assignment on) runs the reference's sequence of framework ops instead, and is the route on the CPU.

Not served, and refused in the constructor: spectral normalisation, ``noise``, and the block types of the future
predictor (cross, cls, ctx, block_causal, skip, skip2).  ``FullAttention`` takes no ``ctx_mask``."""
import torch
import torch.nn as nn

from .. import functional as WF

_FLP_BLOCK_TYPES = ("cross", "cls", "ctx", "block_causal", "skip", "skip2")


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


class FullAttention(_Attention):
    """Self-attention over the tokens of x (B, N, C): models/modules/transform.py:87-122 without ``ctx_mask`` and
    without ``noise``."""

    def __init__(self, dim, num_heads, spectral_norm_layer, noise, **kwargs):
        super().__init__(dim, num_heads, spectral_norm_layer, "FullAttention")
        if noise:
            raise NotImplementedError("FullAttention: noise=True (the LVD networks use False)")
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.proj = nn.Linear(dim, dim)
        self.noise = noise

    def forward(self, x, ctx_mask=None, **kwargs):
        if ctx_mask is not None:
            raise NotImplementedError("FullAttention: ctx_mask (the future predictor's masked clips)")
        q, k, v = self._heads(self.qkv(x), x.shape[0], 3)
        return self.proj(self._attend(q, k, v))


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


class CustomAttention(nn.Module):
    def __init__(self, block_type, **kwargs):
        super().__init__()
        if block_type in ("full", "full_with_cond_norm"):
            self.attn = FullAttention(**kwargs)
        elif block_type == "obj":
            self.attn = ObjAttention(**kwargs)
        elif block_type in _FLP_BLOCK_TYPES:
            raise NotImplementedError(f"CustomAttention: block_type={block_type!r} belongs to the future predictor")
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
