"""Training-clip augmentation on the device, from the packed 8-bit clip (include/waldo_hip.h "Clip augmentation"): what the
reference's ``BaseDataset.__getitem__`` does per frame on the host in PIL and torch -- random zoom and crop, bilinear
resize, flips, colour jitter, normalisation, the resized one-hot layout scaled to +-5 and the flow through its two resizes
(data/base_dataset.py:113-165, :173-208, :330-370) -- in ONE launch that reads the clip's bytes and writes the fp32
sample.

    aug = Augmenter.from_opt(opt)                       # or Augmenter(size, aspect_ratio, true_ratio, max_zoom, ...)
    clip = wio.load_clip(..., packed=True)["vid"].to(dev)
    input, flow = aug(clip, flow=flow, generator=g)     # (B, T, 3 + Nl, H, W) fp32, (B, T, 2, H, W) fp32 or None

The parameters live in device memory (``AugmentParams``): they are drawn there (``sample_params``) and the kernel reads
them there, so a training loop makes no host read, and a HIP graph that holds the launch takes new parameters by an
in-place copy into the tables.  The distributions are the reference's; Python's ``random`` stream is not.  The colour
route is computed in fp32 from the bytes and is NOT bit-equal to the reference's, which rounds to 8 bits after the
resize and after every jitter step.  Contrast jitter, rotation and the fixed-crop branches are
not offered.  There is no CPU fallback."""
import torch

from . import _lib
from .functional import PackedClip, _c, _packed_data

NO_JITTER = 255  # an `order` byte outside 0..5: the frame is not jittered
# order code -> the sequence of operations (0 brightness, 1 saturation, 2 hue): the six permutations, lexicographic
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
FLIP_LR, FLIP_TB = 1, 2  # bits of `flip`: the reference's v_flip (left-right) and h_flip (top-bottom)
# the columns of the uniforms `params_from_uniforms` takes
U_LR, U_TB, U_ZOOM, U_TOP, U_LEFT, U_BRIGHTNESS, U_SATURATION, U_HUE = range(8)


class AugmentParams:
    """The per-clip tables the kernel reads: ``box`` (B, 4) int32 [top, left, h_crop, w_crop] in clip pixels, ``flip``
    (B,) uint8 (bit 0 left-right, bit 1 top-bottom), ``jitter`` (B, 3) fp32 [brightness, saturation, hue], ``order``
    (B, T) uint8 (0..5: ``ORDERS``; 255: no jitter for that frame) and ``zoom`` (B,) fp32, the flow's multiplier."""

    __slots__ = ("box", "flip", "jitter", "order", "zoom")
    _DTYPES = {"box": torch.int32, "flip": torch.uint8, "jitter": torch.float32, "order": torch.uint8,
               "zoom": torch.float32}

    def __init__(self, box, flip, jitter, order, zoom):
        self.box, self.flip, self.jitter, self.order, self.zoom = box, flip, jitter, order, zoom

    def tensors(self):
        return {name: getattr(self, name) for name in self.__slots__}

    def to(self, device, non_blocking=False):
        return AugmentParams(*(t.to(device, non_blocking=non_blocking) for t in self.tensors().values()))

    def copy_(self, other):
        """Overwrite the tables in place (a captured graph reads the same memory at its next replay)."""
        for name, t in self.tensors().items():
            t.copy_(getattr(other, name))
        return self

    def __repr__(self):
        return f"AugmentParams(B={self.box.shape[0]}, T={self.order.shape[1]}, device={self.box.device})"


def params_from_uniforms(u, u_order, *, size, aspect_ratio, true_ratio, max_zoom=1.0, lr_flip=False, tb_flip=False,
                         colorjitter=None, train=True):
    """The default branch of the reference's ``get_augmentation_parameters`` (data/base_dataset.py:114-115, 143-165) on
    given uniforms, as tensor ops in fp64 on ``u``'s device -- no host read.  ``u`` (B, 8) in [0, 1): the columns
    U_LR .. U_HUE, one per ``random.random()`` of the reference; ``u_order`` (B, T) integers in 0..5, the permutation
    ``ColorJitter`` draws at every frame.  ``size``: the clip's (h, w), the reference's (true_dim, int(true_dim
    true_ratio)).  ``train=False``: the evaluation parameters (min_zoom, top = left = 0, no flips, no jitter)."""
    if u.ndim != 2 or u.shape[1] != 8 or u_order.ndim != 2 or u_order.shape[0] != u.shape[0]:
        raise ValueError(f"params_from_uniforms: u must be (B, 8) and u_order (B, T), got {tuple(u.shape)} and "
                         f"{tuple(u_order.shape)}")
    h, w = (int(v) for v in size)
    u = u.to(torch.float64)
    b = u.shape[0]
    min_zoom = max(1.0, aspect_ratio / true_ratio)
    top_zoom = max(max_zoom, min_zoom)
    if train:
        zoom = min_zoom + u[:, U_ZOOM] * (top_zoom - min_zoom)
    else:
        zoom = torch.full((b,), min_zoom, dtype=torch.float64, device=u.device)
    h_crop = torch.trunc(h / zoom)
    w_crop = torch.trunc(h_crop * aspect_ratio)
    if train:
        top = torch.trunc(u[:, U_TOP] * (h - h_crop))
        left = torch.trunc(u[:, U_LEFT] * (w - w_crop))
        flip = ((u[:, U_LR] > 0.5) & bool(lr_flip)).to(torch.uint8) * FLIP_LR
        flip = flip + ((u[:, U_TB] > 0.5) & bool(tb_flip)).to(torch.uint8) * FLIP_TB
    else:
        top = left = torch.zeros_like(zoom)
        flip = torch.zeros(b, dtype=torch.uint8, device=u.device)
    box = torch.stack([top, left, h_crop, w_crop], dim=1).to(torch.int32)
    if colorjitter is not None and train:
        c = float(colorjitter)
        brightness = (1 + (u[:, U_BRIGHTNESS] * 2 - 1) * c).clamp_min(0)
        saturation = (1 + (u[:, U_SATURATION] * 2 - 1) * c).clamp_min(0)
        hue = 0.5 * (u[:, U_HUE] * 2 - 1) * c
        jitter = torch.stack([brightness, saturation, hue], dim=1).to(torch.float32)
        order = u_order.to(torch.uint8)
    else:
        jitter = torch.tensor([1.0, 1.0, 0.0], device=u.device).expand(b, 3).contiguous()
        order = torch.full(tuple(u_order.shape), NO_JITTER, dtype=torch.uint8, device=u.device)
    return AugmentParams(box, flip.contiguous(), jitter, order.contiguous(), zoom.to(torch.float32))


def sample_params(B, T, *, generator=None, device, **fields):
    """Draw the uniforms on ``device`` (``generator``: a generator of that device) and call ``params_from_uniforms``
    with ``fields`` (size, aspect_ratio, true_ratio, max_zoom, lr_flip, tb_flip, colorjitter, train)."""
    u = torch.rand(B, 8, generator=generator, device=device, dtype=torch.float64)
    u_order = torch.randint(0, 6, (B, T), generator=generator, device=device)
    return params_from_uniforms(u, u_order, **fields)


def check_params(params, clip_shape):
    """Host-side validation of the tables against a clip of shape (B, T, C, Hd, Wd): raises ``ValueError``.  It READS the
    tensors -- for CPU tables and tests, not for the training loop (the kernel clamps whatever it is given)."""
    b, t, _, hd, wd = (int(v) for v in clip_shape)
    shapes = {"box": (b, 4), "flip": (b,), "jitter": (b, 3), "order": (b, t), "zoom": (b,)}
    for name, x in params.tensors().items():
        if not torch.is_tensor(x) or x.dtype != AugmentParams._DTYPES[name] or tuple(x.shape) != shapes[name]:
            raise ValueError(f"check_params: {name} must be {AugmentParams._DTYPES[name]} of shape {shapes[name]}, got "
                             f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    box = params.box.cpu().long()
    top, left, hc, wc = box.unbind(1)
    bad = (top < 0) | (left < 0) | (hc < 1) | (wc < 1) | (top + hc > hd) | (left + wc > wd)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise ValueError(f"check_params: box {box[i].tolist()} of clip {i} does not lie inside the {hd} x {wd} clip")
    if (params.flip.cpu() > (FLIP_LR | FLIP_TB)).any():
        raise ValueError("check_params: flip holds bits other than 1 (left-right) and 2 (top-bottom)")
    order = params.order.cpu()
    if ((order > 5) & (order != NO_JITTER)).any():
        raise ValueError(f"check_params: order holds a byte outside 0..5 that is not {NO_JITTER}")
    jitter = params.jitter.cpu()
    if not torch.isfinite(jitter).all() or (jitter[:, :2] < 0).any() or (jitter[:, 2].abs() > 0.5).any():
        raise ValueError("check_params: jitter must be finite with brightness, saturation >= 0 and |hue| <= 0.5")
    zoom = params.zoom.cpu()
    if not torch.isfinite(zoom).all() or (zoom <= 0).any():
        raise ValueError("check_params: zoom must be finite and positive")


def _table(params, name, shape, device):
    x = getattr(params, name)
    if not torch.is_tensor(x) or x.dtype != AugmentParams._DTYPES[name] or tuple(x.shape) != shape:
        raise ValueError(f"augment_clip: params.{name} must be {AugmentParams._DTYPES[name]} of shape {shape}, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if x.device != device:
        raise _lib.WaldoHipError(f"augment_clip: params.{name} is on {x.device}, the clip on {device} (params.to(device))")
    return _c(x)


def _out(x, name, shape, device):
    if x is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not torch.is_tensor(x) or x.dtype != torch.float32 or tuple(x.shape) != shape or not x.is_contiguous() \
            or x.device != device:
        raise ValueError(f"augment_clip: {name} must be a contiguous float32 tensor of shape {shape} on {device}, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    return x


def augment_clip(clip, params, *, flow=None, out_size=None, out=None, flow_out=None):
    """``clip`` (a ``PackedClip`` on the GPU) and ``params`` (``AugmentParams`` on the same device) -> (input, flow):
    ``input`` (B, T, 3 + Nl, Ho, Wo) fp32 in the layout of ``clip.unpack()``, ``flow`` (B, T, 2, Ho, Wo) fp32 or None.
    ``flow``: (B, T, 2, Hf, Wf) fp32, normalised (``tools.io.read_flo``), no larger than the clip.  ``out_size``
    (Ho, Wo): the clip's size when None, never smaller than it.  ``out`` / ``flow_out``: buffers to write into.  One
    ``waldo_augment_clip_fwd`` launch and nothing else on the device; detached."""
    if not isinstance(clip, PackedClip):
        raise ValueError(f"augment_clip: clip must be a PackedClip, got {type(clip).__name__}")
    data = _packed_data(clip, "augment_clip")
    dev = data.device
    b, t, hd, wd, _ = data.shape
    ho, wo = (hd, wd) if out_size is None else (int(v) for v in out_size)
    if ho < hd or wo < wd:
        raise ValueError(f"augment_clip: out_size {(ho, wo)} is smaller than the clip {(hd, wd)}: the resize never "
                         "downsamples (that needs an antialiasing filter)")
    tables = [_table(params, name, shape, dev) for name, shape in
              (("box", (b, 4)), ("flip", (b,)), ("jitter", (b, 3)), ("order", (b, t)), ("zoom", (b,)))]
    hf = wf = 0
    if flow is not None:
        if not torch.is_tensor(flow) or flow.dtype != torch.float32 or flow.ndim != 5 or \
                tuple(flow.shape[:3]) != (b, t, 2):
            raise ValueError(f"augment_clip: flow must be float32 of shape ({b}, {t}, 2, Hf, Wf), got "
                             f"{getattr(flow, 'dtype', type(flow).__name__)} {tuple(getattr(flow, 'shape', ()))}")
        if flow.device != dev:
            raise _lib.WaldoHipError(f"augment_clip: flow is on {flow.device}, the clip on {dev}")
        hf, wf = flow.shape[3:]
        if hf > hd or wf > wd:
            raise ValueError(f"augment_clip: the flow {(hf, wf)} is larger than the clip {(hd, wd)}")
        flow = _c(flow.detach())
        flow_out = _out(flow_out, "flow_out", (b, t, 2, ho, wo), dev)
    elif flow_out is not None:
        raise ValueError("augment_clip: flow_out without a flow")
    out = _out(out, "out", (b, t, 3 + clip.num_lyt, ho, wo), dev)
    box, flip, jitter, order, zoom = tables
    _lib.launch("waldo_augment_clip_fwd", dev, data, flow, box, flip, jitter, order, zoom, out, flow_out, b, t,
                clip.num_lyt, hd, wd, hf, wf, ho, wo)
    return out, flow_out


class Augmenter:
    """``sample_params`` + ``augment_clip`` with the reference's options: ``size`` the sample's (H, W) (None: the
    clip's), ``aspect_ratio`` / ``true_ratio`` / ``max_zoom`` of the zoom and crop, ``lr_flip`` / ``tb_flip`` whether
    each flip is drawn (the reference's ``not no_v_flip`` / ``not no_h_flip``), ``colorjitter`` the jitter's strength
    (None: none).  ``clip_size``: the (h, w) a clip must have (``from_opt``: the size the reference loads), or None."""

    def __init__(self, size=None, aspect_ratio=2.0, true_ratio=2.0, max_zoom=1.0, lr_flip=False, tb_flip=False,
                 colorjitter=None, clip_size=None):
        self.size = None if size is None else tuple(int(v) for v in size)
        self.aspect_ratio, self.true_ratio, self.max_zoom = float(aspect_ratio), float(true_ratio), float(max_zoom)
        self.lr_flip, self.tb_flip = bool(lr_flip), bool(tb_flip)
        self.colorjitter = None if colorjitter is None else float(colorjitter)
        self.clip_size = None if clip_size is None else tuple(int(v) for v in clip_size)

    @classmethod
    def from_opt(cls, opt):
        """From the reference's options (tools/options.py): ``max_zoom``, ``no_v_flip``, ``no_h_flip``, ``colorjitter``,
        ``colorjitter_no_contrast``, ``aspect_ratio``, ``true_ratio``, ``dim``, ``load_dim`` and ``true_dim``.  What the
        kernel does not do is refused with a ``ValueError`` that names the field."""
        for field in ("rotate", "fixed_crop", "fixed_top_centered_zoom"):
            if getattr(opt, field, None):
                raise ValueError(f"Augmenter.from_opt: {field}={getattr(opt, field)!r} is not supported on the device "
                                 "(only the default zoom-and-crop branch is)")
        colorjitter = getattr(opt, "colorjitter", None)
        if colorjitter is not None and not getattr(opt, "colorjitter_no_contrast", False):
            raise ValueError("Augmenter.from_opt: colorjitter_no_contrast must be set: contrast jitter needs the frame's "
                             "mean, a second pass over the frame")
        load = int(opt.dim) if int(getattr(opt, "load_dim", 0)) == 0 else int(opt.load_dim)
        if int(opt.true_dim) != load:
            raise ValueError(f"Augmenter.from_opt: true_dim={opt.true_dim} differs from the load size {load} (dim, or "
                             "load_dim when set): the resize would downsample or the clip is not the recipe's")
        return cls(size=(load, int(load * opt.aspect_ratio)), aspect_ratio=opt.aspect_ratio, true_ratio=opt.true_ratio,
                   max_zoom=opt.max_zoom, lr_flip=not getattr(opt, "no_v_flip", False),
                   tb_flip=not getattr(opt, "no_h_flip", False), colorjitter=colorjitter,
                   clip_size=(int(opt.true_dim), int(opt.true_dim * opt.true_ratio)))

    def params(self, clip, generator=None, train=True):
        b, t, _, hd, wd = clip.shape
        if self.clip_size is not None and (hd, wd) != self.clip_size:
            raise ValueError(f"Augmenter: the clip is {(hd, wd)}, the options say {self.clip_size}")
        return sample_params(b, t, generator=generator, device=clip.device, size=(hd, wd),
                             aspect_ratio=self.aspect_ratio, true_ratio=self.true_ratio, max_zoom=self.max_zoom,
                             lr_flip=self.lr_flip, tb_flip=self.tb_flip, colorjitter=self.colorjitter, train=train)

    def __call__(self, clip, flow=None, generator=None, train=True):
        return augment_clip(clip, self.params(clip, generator, train), flow=flow, out_size=self.size)
