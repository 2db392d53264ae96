"""Drop-in for the reference's ``UNet`` (models/modules/conv.py:28-64): the network in the middle of ``WIF.forward``.

The same constructor signature, forward semantics and parameter names (``to_emb.weight``, ``from_emb.weight``,
``conv_layers.{i}.0.weight``, ``conv_layers.{i}.1.norm.weight|bias``, likewise ``deconv_layers``), so that a reference
checkpoint loads with ``strict=True``.  The convolutions stay the framework's (MIOpen); everything between them -- the
per-plane normalisation (``ln2d`` = GroupNorm with one group per channel), the GELU and the concatenation with the
skip -- is one hand-written kernel per level, ``WF.plane_norm_gelu``.  ``fused = False`` runs the spelled-out
framework ops instead (A/B runs: tools_dev/ab_unet.py).  ``act_dtype = torch.bfloat16 | torch.float16`` runs the
network under autocast with its activations stored in 16 bits, the kernel included."""
import torch
import torch.nn as nn

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
    and the norms keep the framework's defaults."""
    if "Conv2d" in m.__class__.__name__:
        nn.init.xavier_uniform_(m.weight.data, 1.0)


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
