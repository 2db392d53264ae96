"""Renders of the layered decomposition as bytes, made on the device (include/waldo_hip.h "Renders"): which class or
object layer owns a pixel, in class ids or through a palette, and the colour-wheel picture of a flow -- what the
reference's ``Logger.get_lyt`` / ``log_lyt`` (tools/logger.py:169-202 -> ``color_transfer``, tools/utils.py:202-214) and
``Logger.get_flow`` / ``get_flow_rgb`` (tools/logger.py:265-318) make on the host, frame by frame, through matplotlib and
PIL.  The counterpart of ``functional.frames_to_bytes`` for class-like tensors and flows.

    ids = class_ids(output[:, :, 3:3 + Nl])                               # uint8 (B, T, H, W), read in place
    rgb, ids = render_argmax(alpha, layer_palette(L), return_ids=True)    # one launch for both
    pic = render_flow(pred_flow)                                          # uint8 (B, Tc, Tp, 3, H, W)

The colour tables are computed here, in numpy float64, from the closed-form segment definitions of matplotlib's ``jet``
and ``hsv`` maps (matplotlib is not imported); a host table reaches a device once and stays there, so later calls make no
host -> device copy.  Everything is detached; there is no CPU fallback."""
import ctypes

import numpy as np
import torch

from . import _lib
from .functional import BYTE_LAYOUT as LAYOUT
from .functional import BYTE_QUANTIZE as QUANTIZE
from .functional import _DTYPE_CODE, _byte_args, _check_out, _dest, _flat_frames, _frame_stride

MAX_CLASSES = 256  # an id fits a byte
MAX_WHEEL = 4096

# --------------------------------------------------------------------------------------
# Colour tables.  matplotlib's segment data of the two maps: per channel, rows (x, y below x, y above x); a map with N
# entries samples the piecewise-linear function at linspace(0, 1, N) (LinearSegmentedColormap's lookup table, gamma 1).
# --------------------------------------------------------------------------------------
_SEGMENTS = {
    "jet": (
        ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
    ),
    "hsv": (
        ((0., 1., 1.), (0.158730, 1.000000, 1.000000), (0.174603, 0.968750, 0.968750), (0.333333, 0.031250, 0.031250),
         (0.349206, 0.000000, 0.000000), (0.666667, 0.000000, 0.000000), (0.682540, 0.031250, 0.031250),
         (0.841270, 0.968750, 0.968750), (0.857143, 1.000000, 1.000000), (1.0, 1.0, 1.0)),
        ((0., 0., 0.), (0.158730, 0.937500, 0.937500), (0.174603, 1.000000, 1.000000), (0.507937, 1.000000, 1.000000),
         (0.666667, 0.062500, 0.062500), (0.682540, 0.000000, 0.000000), (1.0, 0., 0.)),
        ((0., 0., 0.), (0.333333, 0.000000, 0.000000), (0.349206, 0.062500, 0.062500), (0.507937, 1.000000, 1.000000),
         (0.841270, 1.000000, 1.000000), (0.857143, 0.937500, 0.937500), (1.0, 0.09375, 0.09375)),
    ),
}
_tables = {}


def _channel_table(n, rows):
    """One channel's lookup table with ``n`` entries, in the arithmetic of matplotlib's lookup-table builder (float64)."""
    a = np.array(rows, dtype=np.float64)
    x, y0, y1 = a[:, 0], a[:, 1], a[:, 2]
    if n == 1:  # (the convention for a single entry: the value at the upper end)
        return np.array([y0[-1]])
    x = x * (n - 1)
    xind = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def colormap_table(name, n):
    """The ``n`` RGB entries of matplotlib's ``jet`` or ``hsv`` map with ``n`` entries, float64 (n, 3) -- what
    ``cm.get_cmap(name, n)`` holds, bit for bit (tests compare with matplotlib where it is installed)."""
    n = int(n)
    if name not in _SEGMENTS or n < 1:
        raise ValueError(f"colormap_table: name must be one of {tuple(_SEGMENTS)} and n >= 1, got {name!r}, {n}")
    key = (name, n)
    if key not in _tables:
        t = np.stack([_channel_table(n, rows) for rows in _SEGMENTS[name]], axis=1)
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


def layer_palette(n):
    """The reference's object-layer colours for ``n`` layers (tools/logger.py:176-177), uint8 (n, 3): ``jet`` with n + 1
    entries sampled at ``linspace(0, 1, n + 1)[:n]`` (entry ``int(x * (n + 1))`` of the table, as a colormap called with a
    float does), entry 0 set to grey 0.5, then ``(255 * x).astype(uint8)`` -- the truncation ``color_transfer`` applies."""
    n = int(n)
    if not 1 <= n <= MAX_CLASSES:
        raise ValueError(f"layer_palette: n = {n} outside [1, {MAX_CLASSES}]")
    key = ("layers", n)
    if key not in _tables:
        table = colormap_table("jet", n + 1)
        at = np.linspace(0, 1, n + 1)[:n] * (n + 1)
        cmap = table[np.minimum(at.astype(np.int64), n)].copy()
        cmap[0, :] = 0.5
        pal = (255 * cmap).astype(np.uint8)
        pal.setflags(write=False)
        _tables[key] = pal
    return _tables[key]


def semantic_palette(flat_ints):
    """The bytes the reference shows for a dataset palette given as its option's flat list of 3 * Nl integers
    (tools/logger.py:16-18 -> color_transfer): ``(255 * (p / 255)).astype(uint8)`` in float64, uint8 (Nl, 3).  These are
    the REFERENCE's bytes: where the float64 round trip ``255 * (p / 255)`` falls short of ``p`` the truncation gives one
    below the list's own value."""
    p = np.asarray(flat_ints)
    if p.ndim != 1 or p.size == 0 or p.size % 3 or not np.issubdtype(p.dtype, np.integer) or p.min() < 0 or p.max() > 255:
        raise ValueError("semantic_palette: a flat list of 3 * Nl integers in [0, 255]")
    return (255 * (p.reshape(-1, 3).astype(np.float64) / 255)).astype(np.uint8)


def flow_wheel(k=128):
    """The colour wheel of the reference's flow pictures (tools/logger.py:314): ``hsv`` with ``k`` entries, fp32 (k, 3)."""
    k = int(k)
    if not 1 <= k <= MAX_WHEEL:
        raise ValueError(f"flow_wheel: k = {k} outside [1, {MAX_WHEEL}]")
    return colormap_table("hsv", k).astype(np.float32)


_device_tables = {}


def _on_device(fn, table, device, dtype, what):
    """``table`` (a (rows, 3) array, list or tensor) as a contiguous ``dtype`` tensor on ``device``.  A host table is
    uploaded once per device and content and kept: later calls with the same values copy nothing."""
    if torch.is_tensor(table) and table.is_cuda:
        t = table.detach()
        if t.dtype != dtype or t.ndim != 2 or t.shape[1] != 3:
            raise ValueError(f"{fn}: {what} must be (rows, 3) {dtype}, got {t.dtype} {tuple(t.shape)}")
        if t.device != device:
            raise ValueError(f"{fn}: {what} on {t.device}, the input on {device}")
        return t.contiguous()
    np_dtype = np.uint8 if dtype == torch.uint8 else np.float32
    a = table.detach().numpy() if torch.is_tensor(table) else np.asarray(table)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"{fn}: {what} must be (rows, 3), got {tuple(a.shape)}")
    if np_dtype == np.uint8 and a.dtype != np.uint8:
        if not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
            raise ValueError(f"{fn}: {what} must hold bytes (integers in [0, 255]), got {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np_dtype)
    if device.type != "cuda":
        return torch.from_numpy(a.copy())
    key = (str(device), a.dtype.str, a.shape, a.tobytes())
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(a.copy()).to(device)
    return _device_tables[key]


def _codes(fn, layout, quantize="trunc"):
    _, _, quant, lay = _byte_args(fn, (0.0, 1.0), quantize, layout)
    return lay, quant


def _source(fn, x, what, channels=None):
    """``x`` (..., C, H, W) detached, its leading shape and (C, H, W); refuses what no kernel takes."""
    if not torch.is_tensor(x) or x.ndim < 3 or x.dtype not in _DTYPE_CODE:
        raise ValueError(f"{fn}: {what} must be a (..., C, H, W) float32 / bfloat16 / float16 tensor, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    c, h, w = x.shape[-3:]
    if min(c, h, w) < 1:
        raise ValueError(f"{fn}: empty frames {tuple(x.shape)}")
    if channels is not None and c != channels:
        raise ValueError(f"{fn}: {what} must have {channels} channels (..., {channels}, H, W), got {tuple(x.shape)}")
    if channels is None and c > MAX_CLASSES:
        raise ValueError(f"{fn}: C = {c} classes: an id must fit a byte (C <= {MAX_CLASSES})")
    return x.detach(), tuple(x.shape[:-3]), (c, h, w)


def _need_gpu(fn, x, what):
    if not x.is_cuda:
        raise _lib.WaldoHipError(f"{fn}: {what} must be on the GPU (cuda device); there is no CPU fallback")


def _argmax(fn, x, palette, layout, out, want_ids, ids_out):
    lay, _ = _codes(fn, layout)
    d, lead, (c, h, w) = _source(fn, x, "x")
    want_rgb = palette is not None
    frame = (h, w, 3) if lay else (3, h, w)
    if want_rgb:
        pal = _on_device(fn, palette, d.device, torch.uint8, "palette")
        if pal.shape[0] < c:
            raise ValueError(f"{fn}: the palette has {pal.shape[0]} rows for C = {c} classes")
        _check_out(fn, out, lead, frame)
    _check_out(fn, ids_out, lead, (h, w), "ids")
    _need_gpu(fn, d, "x")
    d = _flat_frames(d)
    n = d.shape[0]
    rgb = _dest(fn, out, n, frame, d.device) if want_rgb else None
    ids = _dest(fn, ids_out, n, (h, w), d.device, "ids") if want_ids else None
    _lib.launch("waldo_render_argmax_fwd", d.device, d, _DTYPE_CODE[d.dtype], d.stride(0), d.stride(1), d.stride(2),
                pal if want_rgb else None, ids, _frame_stride(ids, h * w) if want_ids else 0, rgb,
                _frame_stride(rgb, 3 * h * w) if want_rgb else 0, lay, n, c, h, w)
    rgb_res = (out if out is not None else rgb.view(*lead, *frame)) if want_rgb else None
    ids_res = (ids_out if ids_out is not None else ids.view(*lead, h, w)) if want_ids else None
    return rgb_res, ids_res


def class_ids(x, out=None):
    """The class of every pixel (``waldo_render_argmax_fwd``): ``x`` (..., C, H, W) in fp32, bf16 or fp16 -> uint8
    (..., H, W), the index ``x.float().cpu().max(dim=-3)[1]`` holds -- the lowest channel among the maxima, NaN above
    everything and the first NaN kept.  C <= 256.  ``x`` may be a channel or time slice (``output[:, :, 3:3 + Nl]``): W
    unit-stride, the leading dimensions flattened by stride where possible and copied once otherwise.  With the RGB bytes
    of ``functional.frames_to_bytes`` these ids are the two tensors ``functional.pack_clip`` takes.  ``out``: as
    ``frames_to_bytes``'s.  Detached; no CPU fallback."""
    return _argmax("class_ids", x, None, "nchw", None, True, out)[1]


def render_argmax(x, palette, layout="nchw", out=None, return_ids=False):
    """``palette[class_ids(x)]`` as RGB bytes, uint8 (..., 3, H, W) or with ``layout="nhwc"`` (..., H, W, 3); with
    ``return_ids`` the pair (rgb, ids), both from ONE launch.  ``palette``: at least C rows of 3 bytes -- ``layer_palette``
    / ``semantic_palette``, any (rows, 3) integer array, or a uint8 tensor already on the device (a host table is uploaded
    once and kept).  ``render_argmax(alpha, layer_palette(L))`` is the reference's ``get_lyt(alpha, L)`` mapped to bytes
    (models/synthesizer.py:260, 397).  ``out``: a uint8 tensor of the result's shape to write the RGB bytes into -- dense
    frames, leading dimensions flattenable by stride, any alignment."""
    if palette is None:
        raise ValueError("render_argmax: a palette is needed (class_ids returns the ids alone)")
    rgb, ids = _argmax("render_argmax", x, palette, layout, out, bool(return_ids), None)
    return (rgb, ids) if return_ids else rgb


def render_flow(flow, mul=10.0, wheel=None, quantize="trunc", layout="nchw", out=None):
    """The colour-wheel picture of a flow (``waldo_render_flow_fwd``; the reference's ``Logger.get_flow_rgb``,
    tools/logger.py:310-318, then the library's quantisation with the span (0, 1)): ``flow`` (..., 2, H, W) in fp32, bf16 or
    fp16 -> uint8 (..., 3, H, W) or (..., H, W, 3).  Brightness ``min(|flow| / sqrt(2) * mul, 1)``, hue the entry
    ``int(theta * K)`` of ``wheel`` (default ``flow_wheel(128)``; fp32 (K, 3), K <= 4096) at
    ``theta = (1 + atan2(v, u) / pi) / 2``.  NaN and a zero flow give bytes 0.  ``quantize``, ``layout``, ``out``: as
    ``functional.frames_to_bytes``'s."""
    fn = "render_flow"
    lay, quant = _codes(fn, layout, quantize)
    d, lead, (_, h, w) = _source(fn, flow, "flow", channels=2)
    mul = ctypes.c_float(float(mul)).value
    if not np.isfinite(mul):
        raise ValueError(f"{fn}: mul must be finite, got {mul}")
    tab = _on_device(fn, flow_wheel() if wheel is None else wheel, d.device, torch.float32, "wheel")
    if tab.shape[0] > MAX_WHEEL:
        raise ValueError(f"{fn}: the wheel has {tab.shape[0]} rows (at most {MAX_WHEEL})")
    frame = (h, w, 3) if lay else (3, h, w)
    _check_out(fn, out, lead, frame)
    _need_gpu(fn, d, "flow")
    d = _flat_frames(d)
    n = d.shape[0]
    o = _dest(fn, out, n, frame, d.device)
    _lib.launch("waldo_render_flow_fwd", d.device, d, _DTYPE_CODE[d.dtype], d.stride(0), d.stride(1), d.stride(2), tab,
                tab.shape[0], mul, o, _frame_stride(o, 3 * h * w), lay, quant, n, h, w)
    return out if out is not None else o.view(*lead, *frame)
