"""Drop-in for the reference's ``UNet`` (models/modules/conv.py:28-64): the network in the middle of ``WIF.forward``.

The same constructor signature, forward semantics and parameter names (``to_emb.weight``, ``from_emb.weight``,
``conv_layers.{i}.0.weight``, ``conv_layers.{i}.1.norm.weight|bias``, likewise ``deconv_layers``), so that a reference
checkpoint loads with ``strict=True``.  The convolutions stay the framework's (MIOpen); everything between them -- the
per-plane normalisation (``ln2d`` = GroupNorm with one group per channel), the GELU and the concatenation with the
skip -- is one hand-written kernel per level, ``WF.plane_norm_gelu``.  ``fused = False`` runs the spelled-out
framework ops instead (A/B runs: tools_dev/ab_unet.py).  ``act_dtype = torch.bfloat16 | torch.float16`` runs the
network under autocast with its activations stored in 16 bits, the kernel included.

``ConvPatchProj`` (models/modules/conv.py:67-180), the patch embedding of the LVD encoder and decoders, is built from the
same conv -> norm -> GELU triple and runs it through the same kernel."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as WF


_KERNEL = dict(kernel_size=3, padding=1, bias=False)  # every convolution of the network: 3 x 3, padded, no bias


def _same_size_conv(cin, cout):
    """The two stride-1 convolutions at the ends (``to_emb``, ``from_emb``)."""
    return nn.Conv2d(cin, cout, **_KERNEL)


class CustomNorm(nn.Module):
    """The two norms a UNet is built with: ``ln2d`` (GroupNorm(dim, dim): statistics per (n, c) plane) and ``bn2d``
    (SyncBatchNorm).  The norm lives under ``.norm``, as in the reference's state dict."""

    def __init__(self, norm_layer, dim):
        super().__init__()
        self.norm_type = norm_layer
        if norm_layer == "ln2d":
            self.norm = nn.GroupNorm(dim, dim)
        elif norm_layer == "bn2d":
            self.norm = nn.SyncBatchNorm(dim)
        else:
            raise ValueError(f"UNet: norm_layer must be 'ln2d' or 'bn2d', got {norm_layer!r}")

    def forward(self, x):
        return self.norm(x)


def _make_level(cin, cout, norm_layer, up):
    """One level as the reference's state dict indexes it: [0] the stride-2 convolution -- transposed, with
    ``output_padding=1`` (exactly twice the size), when ``up`` -- [1] the norm, [2] the GELU."""
    if up:
        resample = nn.ConvTranspose2d(cin, cout, stride=2, output_padding=1, **_KERNEL)
    else:
        resample = nn.Conv2d(cin, cout, stride=2, **_KERNEL)
    return nn.Sequential(resample, CustomNorm(norm_layer, cout), nn.GELU())


def init_weights(m):
    """The reference's rule (models/modules/weight_init.py:70-81) for the modules of a UNet: Xavier-uniform, gain 1,
    for every module whose class name contains "Conv2d" -- which ConvTranspose2d does not: the transposed convolutions
    and the plane norms keep the framework's defaults; a Linear gets a truncated normal (std 0.02, cut at +-2) and a zero
    bias, a LayerNorm weight 1 and bias 0."""
    if "Conv2d" in m.__class__.__name__:
        nn.init.xavier_uniform_(m.weight.data, 1.0)
    elif isinstance(m, nn.Linear):  # (the token networks of nets.lvd: a UNet has none)
        nn.init.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.zeros_(m.bias)
    elif isinstance(m, nn.LayerNorm) and m.elementwise_affine:
        nn.init.ones_(m.weight)
        if m.bias is not None:
            nn.init.zeros_(m.bias)


class UNet(nn.Module):
    def __init__(self, num_channels_in, num_channels_out, embed_dim, norm_layer, depth, scale_hd, zero_init, upmode):
        super().__init__()  # (scale_hd and upmode: accepted and unused, as in the reference)
        self.depth = depth
        self.fused = True  # False: GroupNorm, GELU and cat as framework ops
        self.act_dtype = None
        base = embed_dim // (2 ** (depth - 1))
        self.to_emb = _same_size_conv(num_channels_in, base)
        self.from_emb = _same_size_conv(2 * base, num_channels_out)
        widths = [base << i for i in range(depth)]  # level i works at width base * 2^i: down to twice it, up from it
        self.conv_layers = nn.ModuleList(_make_level(wd, 2 * wd, norm_layer, up=False) for wd in widths)
        # an up level takes the level below (twice its width) concatenated with that level's skip; the last has no skip
        self.deconv_layers = nn.ModuleList(_make_level((2 if i == depth - 1 else 4) * wd, wd, norm_layer, up=True)
                                           for i, wd in enumerate(widths))
        self.apply(init_weights)
        if zero_init:
            self.from_emb.weight.data.zero_()

    @property
    def act_dtype(self):
        """None: the caller's precision.  torch.bfloat16 / torch.float16: ``forward`` runs inside
        ``torch.autocast(x.device.type, dtype=act_dtype)`` -- fp32 master weights, 16-bit convolutions -- every fused
        level stores its activations in that type (``WF.plane_norm_gelu(..., out_dtype=act_dtype)``: no fp32 copy of
        a level crosses memory), and the output is of that type.  With ``fused = False`` the same region is the
        framework's autocast route (GroupNorm in fp32, rounded by the next convolution)."""
        return self._act_dtype

    @act_dtype.setter
    def act_dtype(self, dtype):
        if dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError(f"UNet: act_dtype must be None, torch.bfloat16 or torch.float16, got {dtype!r}")
        self._act_dtype = dtype

    def _level(self, layer, x, skip=None):
        """conv -> norm -> GELU (-> cat with ``skip``) of one level."""
        y = layer[0](x)
        norm = layer[1].norm
        if self.fused and isinstance(norm, nn.GroupNorm) and norm.num_groups == norm.num_channels:
            return WF.plane_norm_gelu(y, norm.weight, norm.bias, skip, norm.eps, out_dtype=self._act_dtype)
        y = layer[2](layer[1](y))
        return y if skip is None else torch.cat([y, skip], dim=1)

    def forward(self, x):
        if x.dim() != 4 or x.shape[-2] % (1 << self.depth) or x.shape[-1] % (1 << self.depth):
            raise ValueError(f"UNet: H and W must be multiples of 2**depth = {1 << self.depth} (the skips of the "
                             f"{self.depth} stride-2 levels would not line up), got {tuple(x.shape)}")
        if self._act_dtype is None:
            return self._forward(x)
        with torch.autocast(x.device.type, dtype=self._act_dtype):
            return self._forward(x)

    def _forward(self, x):
        ys = [self.to_emb(x)]
        for i in range(self.depth):
            ys.append(self._level(self.conv_layers[i], ys[-1]))
        y = ys.pop()
        for i in range(self.depth):
            y = self._level(self.deconv_layers[-1 - i], y, ys.pop())
        return self.from_emb(y)


def _resample(cin, cout, up):
    """A stride-2 convolution of the patch projections: halves the raster, or (transposed) doubles it exactly."""
    if up:
        return nn.ConvTranspose2d(cin, cout, stride=2, output_padding=1, **_KERNEL)
    return nn.Conv2d(cin, cout, stride=2, **_KERNEL)


class ConvPatchProj(nn.Module):
    """Drop-in for the reference's ``ConvPatchProj`` (models/modules/conv.py:67-180): the convolutional patch embedding
    of the LVD encoder (``from_patch=True``: image (B, C, H, W) -> tokens (B, H W / patch^2, embed)) and its mirror in
    the decoders (``from_patch=False``: tokens (B, L, embed) with ``latent_shape`` -> image).  log2(patch_size) stride-2
    steps between widths embed, embed / 2, ..., num_channels; every step but the one at the image end (``proj``) is
    conv -> ``ln2d`` -> GELU.  Same signature and parameter names (``layers.{i}.0.weight``,
    ``layers.{i}.1.norm.weight|bias``, ``proj.weight``, ``skip_proj.weight``, ``hr_layers.*``, ``hr_proj.weight``).

    The conv -> norm -> GELU triples run as the framework's convolution followed by ONE kernel,
    ``WF.plane_norm_gelu`` (``fused = False``: the framework's GroupNorm and GELU; also the route of CPU tensors).
    ``use_hr``, ``x_list`` / ``fuse_m`` and ``skip`` are served with framework ops."""

    def __init__(self, patch_size, embed_dim, norm_layer, num_channels, skip_channels=0, from_patch=True, hr_ratio=None,
                 use_hr=False):
        super().__init__()
        self.from_patch = from_patch
        self.num_channels = num_channels
        self.use_hr = use_hr
        self.norm_layer = norm_layer
        self.patch_size = patch_size
        self.use_skip = skip_channels > 0
        self.fused = True
        steps = int(math.log2(patch_size))
        # widths from the token end to the image end
        widths = [embed_dim >> k for k in range(steps)] + [num_channels]
        hr_widths = []
        if use_hr:
            if hr_ratio is None:
                raise ValueError("ConvPatchProj: use_hr needs hr_ratio")
            hr_widths = [embed_dim >> k for k in range(steps - 1, steps + int(math.log2(hr_ratio)))] + [num_channels]
        self.layers, proj_io = self._stack(widths)
        if self.use_skip:
            if from_patch or use_hr:
                raise NotImplementedError("ConvPatchProj: skip_channels with from_patch or use_hr")
            self.skip_proj = _resample(skip_channels, proj_io[0], up=False)
            proj_io = (2 * proj_io[0], proj_io[1])
        self.proj = _resample(*proj_io, up=not from_patch)
        if use_hr:
            self.hr_layers, hr_io = self._stack(hr_widths)
            self.hr_proj = _resample(*hr_io, up=not from_patch)

    def _stack(self, widths):
        """(the ModuleList of the steps between ``widths`` that are not the image-end projection, that projection's
        (cin, cout)).  Towards the tokens (from_patch) the LAST step of the list is a bare convolution; towards the
        image every step of the list is activated."""
        up = not self.from_patch
        if self.from_patch:
            widths = widths[::-1]
            inner, proj_io = widths[1:], tuple(widths[:2])
        else:
            inner, proj_io = widths[:-1], tuple(widths[-2:])
        activated = len(inner) - 1 if up else len(inner) - 2
        layers = [nn.Sequential(_resample(inner[i], inner[i + 1], up), CustomNorm(self.norm_layer, inner[i + 1]), nn.GELU())
                  for i in range(activated)]
        if not up:
            layers.append(_resample(inner[-2], inner[-1], up))
        return nn.ModuleList(layers), proj_io

    def _step(self, layer, x):
        if isinstance(layer, nn.Sequential):
            norm = layer[1].norm
            if self.fused and isinstance(norm, nn.GroupNorm) and norm.num_groups == norm.num_channels:
                return WF.plane_norm_gelu(layer[0](x), norm.weight, norm.bias, None, norm.eps)
        return layer(x)

    @staticmethod
    def _blend(x, x_list, idx, fuse_m):
        """``fuse_m * x_list[idx] + (1 - fuse_m) * x`` with the mask resized to x's raster; no list: x."""
        if x_list is not None:
            m = F.interpolate(fuse_m, size=x.shape[-2:], mode="bilinear", align_corners=False)
            x = m * x_list[idx] + (1 - m) * x
        return x, idx + 1

    def forward(self, x, latent_shape=None, return_list=False, x_list=None, fuse_m=None, skip=None):
        if self.from_patch:
            kept = []
            c = x.shape[1]
            if c == self.num_channels - 1:    # an alpha channel is expected and absent: opaque
                x = torch.cat([x, torch.ones_like(x[:, :1])], dim=1)
            if c == self.num_channels + 1:    # an alpha channel is present and not expected: dropped
                x = x[:, :self.num_channels]
            x = self.hr_proj(x) if self.use_hr else self.proj(x)
            kept.append(x)
            for layer in (list(self.hr_layers) if self.use_hr else []) + list(self.layers):
                x = self._step(layer, x)
                kept.append(x)
            if return_list:
                return kept[::-1]
            return x.flatten(2).transpose(1, 2).contiguous()
        if latent_shape is None:
            raise ValueError("ConvPatchProj: tokens need latent_shape")
        b, _, c = x.shape
        h, w = latent_shape
        x = x.view(b, h, w, c).permute(0, 3, 1, 2).contiguous()
        idx = 0
        for layer in list(self.layers) + (list(self.hr_layers) if self.use_hr else []):
            x, idx = self._blend(x, x_list, idx, fuse_m)
            x = self._step(layer, x)
        x, idx = self._blend(x, x_list, idx, fuse_m)
        if self.use_hr:
            return self.hr_proj(x)
        if self.use_skip:
            x = torch.cat([x, self.skip_proj(skip)], dim=1)
        return self.proj(x)
