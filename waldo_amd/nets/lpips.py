"""LPIPS (Zhang et al., "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric"), the ``lpips`` package's
``LPIPS(net=..., lpips=True)`` in eval mode: the reference's ``lpips_vid`` loss (``net="vgg"``, models/synthesizer.py:597-600)
and its evaluation's headline metric (``net="alex"``, tools/eval/metrics.py:127).

A scaling layer, a convolutional backbone tapped after five ReLUs, and at each tap ``WF.lpips_level`` with that level's
lin weights (include/waldo_hip.h "LPIPS level distance": one fused kernel pair in place of the chain of elementwise and
reduction ops); the five levels add up.  The convolutions stay on the framework's library.  The module, its parameter
names and its state-dict layout follow the package's published structure, so that a saved ``lpips.LPIPS`` state dict
loads strictly -- the weights themselves are NOT shipped: ``LPIPS.load`` takes them from the user's files.  The module
has not been run against the package or its weights.
"""
import torch
import torch.nn as nn

from .. import functional as WF

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# per net: the five slices as (index in torchvision's ``features``, layer); "C" (in, out, kernel, stride, pad), "R" a
# ReLU, "M" (kernel, stride) a max pool.  A tap follows each slice.
_VGG = (
    ((0, ("C", 3, 64, 3, 1, 1)), (1, "R"), (2, ("C", 64, 64, 3, 1, 1)), (3, "R")),
    ((4, ("M", 2, 2)), (5, ("C", 64, 128, 3, 1, 1)), (6, "R"), (7, ("C", 128, 128, 3, 1, 1)), (8, "R")),
    ((9, ("M", 2, 2)), (10, ("C", 128, 256, 3, 1, 1)), (11, "R"), (12, ("C", 256, 256, 3, 1, 1)), (13, "R"),
     (14, ("C", 256, 256, 3, 1, 1)), (15, "R")),
    ((16, ("M", 2, 2)), (17, ("C", 256, 512, 3, 1, 1)), (18, "R"), (19, ("C", 512, 512, 3, 1, 1)), (20, "R"),
     (21, ("C", 512, 512, 3, 1, 1)), (22, "R")),
    ((23, ("M", 2, 2)), (24, ("C", 512, 512, 3, 1, 1)), (25, "R"), (26, ("C", 512, 512, 3, 1, 1)), (27, "R"),
     (28, ("C", 512, 512, 3, 1, 1)), (29, "R")),
)
_ALEX = (
    ((0, ("C", 3, 64, 11, 4, 2)), (1, "R")),
    ((2, ("M", 3, 2)), (3, ("C", 64, 192, 5, 1, 2)), (4, "R")),
    ((5, ("M", 3, 2)), (6, ("C", 192, 384, 3, 1, 1)), (7, "R")),
    ((8, ("C", 384, 256, 3, 1, 1)), (9, "R")),
    ((10, ("C", 256, 256, 3, 1, 1)), (11, "R")),
)
NETS = {"vgg": _VGG, "alex": _ALEX}
TAP_WIDTHS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}


def _layer(spec):
    if spec == "R":
        return nn.ReLU(inplace=True)
    if spec[0] == "M":
        return nn.MaxPool2d(kernel_size=spec[1], stride=spec[2])
    _, cin, cout, k, s, p = spec
    return nn.Conv2d(cin, cout, k, stride=s, padding=p)


class _Backbone(nn.Module):
    def __init__(self, slices):
        super().__init__()
        for k, layers in enumerate(slices):
            seq = nn.Sequential()
            for idx, spec in layers:
                seq.add_module(str(idx), _layer(spec))
            setattr(self, f"slice{k + 1}", seq)


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))

    def forward(self, x):
        return (x - self.shift) / self.scale


class _Lin(nn.Module):
    """The package's ``NetLinLayer``: a dropout (the identity in eval mode: index 0) and a bias-free 1 x 1 convolution
    to one channel (index 1).  Only its weight is used: ``WF.lpips_level`` applies it."""

    def __init__(self, channels):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(channels, 1, 1, bias=False))


def _read(source, what):
    if source is None or isinstance(source, dict):
        return source
    state = torch.load(source, map_location="cpu", weights_only=True)
    if not isinstance(state, dict):
        raise ValueError(f"LPIPS.load: {what} {source!r} does not hold a state dict")
    return state


class LPIPS(nn.Module):
    """``forward(in0, in1, normalize=False)`` -> (N, 1, 1, 1): the distance of each image pair.  Inputs are (N, 3, H, W)
    in [-1, 1]; ``normalize=True`` takes them in [0, 1].  ``net``: ``"vgg"`` (the loss) or ``"alex"`` (the metric).
    ``fused=False`` runs every level in framework ops (``WF.lpips_level_framework``: the A/B and the tests).  At most
    ``chunk`` image pairs go through the backbone at a time; the per-image results do not depend on it.  Always in eval
    mode with frozen parameters: gradients reach the inputs only.  A new module holds RANDOM weights (He-normal
    convolutions, non-negative lin weights) drawn from ``generator`` (a ``torch.Generator``; the global one when None):
    ``LPIPS.load`` builds one from files.

    ``act_dtype`` (None, ``torch.bfloat16`` or ``torch.float16``): the backbone's activations in 16 bits.  The scaling
    layer stays fp32, the backbone slices run under ``torch.autocast`` of that type (fp32 parameters, 16-bit taps), and
    each tap goes -- outside the autocast region -- to ``WF.lpips_level`` with the fp32 lin weights: the 16-bit level
    kernels (fp32 arithmetic, fp32 level sums, an fp32 result).  With ``fused=False`` the taps are widened to fp32 for
    ``WF.lpips_level_framework``.  fp16 gradients of a mean over many pixels are small: scale the loss.  None: the fp32
    module."""

    def __init__(self, net="vgg", fused=True, chunk=8, spatial=False, generator=None, act_dtype=None):
        super().__init__()
        if act_dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError(f"LPIPS: act_dtype must be None, torch.bfloat16 or torch.float16, got {act_dtype!r}")
        self.act_dtype = act_dtype
        if net not in NETS:
            raise ValueError(f"LPIPS: net must be one of {tuple(NETS)}, got {net!r} (the squeeze backbone is not served)")
        if spatial:
            raise ValueError("LPIPS: spatial=True is not served (the distance is averaged over the pixels)")
        if int(chunk) < 1:
            raise ValueError(f"LPIPS: chunk must be >= 1, got {chunk}")
        self.net_name, self.fused, self.chunk = net, bool(fused), int(chunk)
        self.scaling_layer = _ScalingLayer()
        self.net = _Backbone(NETS[net])
        for k, c in enumerate(TAP_WIDTHS[net]):
            setattr(self, f"lin{k}", _Lin(c))
        for m in self.net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu", generator=generator)
                nn.init.zeros_(m.bias)
        for k, c in enumerate(TAP_WIDTHS[net]):
            nn.init.uniform_(self.lin(k), 0.0, 2.0 / c, generator=generator)
        self.requires_grad_(False)
        super().train(False)

    def lin(self, k):
        return getattr(self, f"lin{k}").model[1].weight

    def train(self, mode=True):
        """Eval mode is the only mode served: the call changes nothing."""
        return self

    @classmethod
    def load(cls, net, state=None, backbone=None, lin=None, **kwargs):
        """A module with the user's weights.  Either ``state``: a full ``lpips.LPIPS`` state dict (with or without the
        package's ``lins.{k}.model.1.weight`` aliases of ``lin{k}.model.1.weight``); or ``backbone`` + ``lin``: a
        torchvision ``vgg16`` / ``alexnet`` state dict (``features.{i}.weight|bias``; the classifier's keys are ignored)
        and the package's lin file (``lin{k}.model.1.weight``).  Each a dict or a file ``torch.save`` wrote.  Any other
        unknown key, or a missing one, is a ``KeyError`` that names it."""
        if (state is None) == (backbone is None and lin is None) or (backbone is None) != (lin is None):
            raise ValueError("LPIPS.load: pass either state=, or backbone= together with lin=")
        module = cls(net, **kwargs)
        own = module.state_dict()
        if state is not None:
            given = dict(_read(state, "state"))
            for k in range(5):
                alias, name = f"lins.{k}.model.1.weight", f"lin{k}.model.1.weight"
                if alias in given:
                    twin = given.pop(alias)
                    if name in given and not torch.equal(twin, given[name]):
                        raise KeyError(f"LPIPS.load: {alias} and {name} hold different tensors")
                    given.setdefault(name, twin)
        else:
            given = {}
            index_of = {name.split(".")[2]: name.rsplit(".", 1)[0] for name in own if name.startswith("net.")}
            for key, value in _read(backbone, "backbone").items():
                part = key.split(".")
                if part[0] == "classifier":
                    continue
                if len(part) != 3 or part[0] != "features" or part[1] not in index_of or part[2] not in ("weight", "bias"):
                    raise KeyError(f"LPIPS.load: unknown key {key!r} in the backbone file")
                given[f"{index_of[part[1]]}.{part[2]}"] = value
            for key, value in _read(lin, "lin").items():
                if key not in own or not key.startswith("lin"):
                    raise KeyError(f"LPIPS.load: unknown key {key!r} in the lin file")
                given[key] = value
            for name in ("scaling_layer.shift", "scaling_layer.scale"):
                given[name] = own[name]
        for key in given:
            if key not in own:
                raise KeyError(f"LPIPS.load: unknown key {key!r}")
        for key, value in own.items():
            if key not in given:
                raise KeyError(f"LPIPS.load: missing key {key!r}")
            if tuple(given[key].shape) != tuple(value.shape):
                raise KeyError(f"LPIPS.load: {key!r} has shape {tuple(given[key].shape)}, expected {tuple(value.shape)}")
        module.load_state_dict(given, strict=True)
        return module

    def _pairs(self, in0, in1):
        """(n,) distances of one chunk: both images through the backbone slice by slice, a level distance per tap."""
        level = WF.lpips_level if self.fused else WF.lpips_level_framework
        a, b = self.scaling_layer(in0), self.scaling_layer(in1)
        total = None
        for k in range(5):
            piece = getattr(self.net, f"slice{k + 1}")
            if self.act_dtype is None:
                a, b = piece(a), piece(b)
                d = level(a, b, self.lin(k))
            else:
                with torch.autocast(in0.device.type, dtype=self.act_dtype):
                    a, b = piece(a), piece(b)
                d = level(a, b, self.lin(k)) if self.fused else level(a.float(), b.float(), self.lin(k))
            total = d if total is None else total + d
        return total

    def forward(self, in0, in1, normalize=False):
        for name, x in (("in0", in0), ("in1", in1)):
            if not torch.is_tensor(x) or x.ndim != 4 or x.shape[1] != 3 or not x.is_floating_point():
                raise ValueError(f"LPIPS: {name} must be a floating (N, 3, H, W) tensor, got "
                                 f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
        if in0.shape != in1.shape:
            raise ValueError(f"LPIPS: in0 {tuple(in0.shape)} and in1 {tuple(in1.shape)} differ in shape")
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        n = in0.shape[0]
        outs = [self._pairs(in0[s:s + self.chunk], in1[s:s + self.chunk]) for s in range(0, n, self.chunk)]
        return (outs[0] if len(outs) == 1 else torch.cat(outs)).view(n, 1, 1, 1)
