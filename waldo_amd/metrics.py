"""Scores of predicted clips: PSNR, SSIM and MS-SSIM per frame on the device, and the reference's aggregation.

The reference scores its dumped mp4 clips with TensorFlow (tools/eval/metrics.py:67-74: ``tf.image.psnr``,
``tf.image.ssim``, ``tf.image.ssim_multiscale`` with ``max_val=1`` on frames of ``uint8 / 255.``).  ``frame_metrics``
computes the same definitions with the gfx950 kernels of ``csrc/frame_metrics.hip`` (include/waldo_hip.h "Frame
metrics"):

- SSIM: the 11 x 11 Gaussian window (sigma 1.5), VALID correlation, ``c1 = 0.01^2``, ``c2 = 0.03^2``; the mean of
  ``lum * cs`` over the VALID map, then over the 3 channels.
- MS-SSIM: 5 scales weighted ``(0.0448, 0.2856, 0.3001, 0.2363, 0.1333)``; each scale the 2 x 2 average of the one
  before, an odd side padded at its end by repeating the last row / column; ``prod relu(cs_k)^w_k`` below the last
  scale times ``relu(ssim_4)^w_4``, averaged over the channels.  Every scale must be at least 11 x 11: H, W >= 161.
- PSNR: ``-10 log10(mse)`` over all pixels and channels, ``+inf`` for equal frames.

- LPIPS (the reference's ``lpips_tf.lpips(..., model='net-lin', net='alex')`` on frames in [0, 1] mapped to [-1, 1],
  tools/eval/metrics.py:127): with ``lpips=`` a ``waldo_amd.nets.LPIPS`` module, through its backbone and the fused
  level kernel (include/waldo_hip.h "LPIPS level distance").  Its pretrained weights are not shipped: the caller loads
  them (``LPIPS.load``), and without a module the metric is refused.  Agreement with the ``lpips`` package's own
  weights and outputs has not been verified.

Not covered: the reference's ``--compress`` / ``--resize`` (cv2 ``INTER_LINEAR``) and reading mp4 files.
"""
import numpy as np
import torch

from . import _lib
from .functional import PackedClip, rgb_table

METRICS = ("psnr", "ssim", "msssim")
_BITS = {"psnr": 1, "ssim": 2, "msssim": 4}  # WALDO_METRIC_*
QUANTIZE = {"trunc": 0, "round": 1, "none": 2}  # WALDO_METRICS_TRUNC / _ROUND / _NONE
_ENC_F32, _ENC_U8, _ENC_PACKED = 0, 1, 2
MIN_SSIM_SIDE = 11  # the window
MIN_MSSSIM_SIDE = 161  # 161 -> 81 -> 41 -> 21 -> 11: the smallest side whose fifth scale holds the window


def _scales_ok(side, n):
    for _ in range(n - 1):
        side = (side + 1) // 2
    return side >= MIN_SSIM_SIDE


def _operand_shape(x, name):
    if isinstance(x, PackedClip):
        b, t, _, h, w = x.shape
        return (b, t, h, w)
    if not torch.is_tensor(x) or x.ndim != 5 or x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"frame_metrics: {name} must be a (B, T, 3, H, W) float32 or uint8 tensor or a PackedClip, "
                         f"got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if x.shape[2] != 3:
        raise ValueError(f"frame_metrics: {name} has {x.shape[2]} channels, the metrics take 3 (RGB): "
                         "slice the clip, e.g. clip[:, :, :3]")
    b, t, _, h, w = x.shape
    return (b, t, h, w)


def _descriptor(x):
    """(tensor kept alive, encoding, strides b, t, c, h) of an operand on the GPU."""
    if isinstance(x, PackedClip):
        d = x.data
        if d.stride(-1) != 1 or d.stride(-2) != 4 or d.data_ptr() % 4:
            d = d.contiguous()
        return d, _ENC_PACKED, (d.stride(0) // 4, d.stride(1) // 4, 0, d.stride(2) // 4)
    d = x.detach()
    if d.stride(-1) != 1:
        d = d.contiguous()
    enc = _ENC_F32 if d.dtype == torch.float32 else _ENC_U8
    return d, enc, (d.stride(0), d.stride(1), d.stride(2), d.stride(3))


def check_metrics(metrics, lpips=None):
    """The metric names as a tuple; ValueError for an unknown one, and for ``"lpips"`` without an ``LPIPS`` module (its
    weights are not shipped: the caller loads them)."""
    metrics = tuple(metrics)
    if not metrics:
        raise ValueError("frame_metrics: no metric asked for")
    for m in metrics:
        if m == "lpips" and lpips is not None:
            if not callable(lpips):
                raise ValueError(f"frame_metrics: lpips= must be an LPIPS module, got {type(lpips).__name__}")
            continue
        if m == "lpips":
            raise ValueError("frame_metrics: 'lpips' is not available: it needs the pretrained AlexNet and LPIPS "
                             "linear-layer weights (alexnet / net-lin), which are not shipped with this library")
        if m not in _BITS:
            raise ValueError(f"frame_metrics: unknown metric {m!r}; choose from {METRICS}")
    return metrics


def _unit_frames(x, lo, hi, quantize):
    """A dense clip as the [0, 1] values the metrics see (``frame_metrics``'s ``quantize``), flattened to frames."""
    if x.dtype == torch.uint8:
        return x.flatten(0, 1).float() / 255.0
    u = ((x.flatten(0, 1) - lo) / (hi - lo)).clamp(0.0, 1.0)
    if quantize == "none":
        return u
    return torch.trunc(u * 255.0 + (0.5 if quantize == "round" else 0.0)) / 255.0


def frame_metrics(pred, real, metrics=METRICS, span=(-1.0, 1.0), quantize="trunc", lpips=None):
    """Per-frame scores of ``pred`` against ``real``: a dict metric name -> (B, T) float32 tensor on the device.

    Each operand is a (B, T, 3, H, W) float32 clip with values in ``span`` (any strides for B, T and C; W unit-stride,
    so ``rec_output[:, :, :3]`` needs no copy), a (B, T, 3, H, W) uint8 clip (bytes, taken as they are), or a
    ``PackedClip`` (its RGB bytes, read in place; it stands for its unpacked fp32 form, as everywhere in the library).
    ``quantize`` maps an fp32 value (and a packed clip's ``rgb_table`` value) to [0, 1], after
    ``u = clamp((x - lo) / (hi - lo), 0, 1)``:

    - ``"trunc"``: ``trunc(u * 255) / 255``, the bytes the reference's ``dump_video`` writes (tools/utils.py:246-264)
      -- the default, as the reference scores its dumped clips;
    - ``"round"``: ``trunc(u * 255 + 0.5) / 255``, the bytes ``tools.io.dump_video`` / ``dump_image`` write;
    - ``"none"``: ``u`` itself.

    ``lpips``: a ``waldo_amd.nets.LPIPS`` module on the operands' device; with it ``"lpips"`` may be asked for, and the
    result gains ``"lpips"``: the module applied to ``2 u - 1`` of both clips' frames, ``u`` the [0, 1] values above
    (bytes: ``x / 255``), under ``no_grad``, ``lpips.chunk`` frames at a time.  Dense operands only.

    Raises ``ValueError`` for shapes that differ, channels other than 3, a frame below a metric's size limit
    (SSIM 11 x 11, MS-SSIM 161 x 161), ``"lpips"`` without a module or with a ``PackedClip``; ``WaldoHipError`` for
    operands that are not on the GPU.
    Deterministic: two calls, and ``frame_metrics(a, b)`` / ``frame_metrics(b, a)``, give the same bits."""
    metrics = check_metrics(metrics, lpips)
    if quantize not in QUANTIZE:
        raise ValueError(f"frame_metrics: quantize must be one of {tuple(QUANTIZE)}, got {quantize!r}")
    lo, hi = (float(v) for v in span)
    if not hi > lo:
        raise ValueError(f"frame_metrics: span {span} must have lo < hi")
    shp = _operand_shape(pred, "pred")
    if _operand_shape(real, "real") != shp:
        raise ValueError(f"frame_metrics: pred and real differ in shape: {tuple(pred.shape)} vs {tuple(real.shape)}")
    b, t, h, w = shp
    if "lpips" in metrics and (isinstance(pred, PackedClip) or isinstance(real, PackedClip)):
        raise ValueError("frame_metrics: 'lpips' takes dense (B, T, 3, H, W) clips, not a PackedClip: unpack_clip it")
    mask = 0
    for m in metrics:
        mask |= _BITS.get(m, 0)
    if "msssim" in metrics and not (_scales_ok(h, 5) and _scales_ok(w, 5)):
        raise ValueError(f"frame_metrics: msssim needs 5 scales of at least 11x11, and {h}x{w} has "
                         f"{(h + 15) // 16}x{(w + 15) // 16} at the last: the smallest frame that works is "
                         f"{MIN_MSSSIM_SIDE}x{MIN_MSSSIM_SIDE}")
    if "ssim" in metrics and min(h, w) < MIN_SSIM_SIDE:
        raise ValueError(f"frame_metrics: ssim needs frames of at least {MIN_SSIM_SIDE}x{MIN_SSIM_SIDE}, got {h}x{w}")
    for name, x in (("pred", pred), ("real", real)):
        if not x.is_cuda:
            raise _lib.WaldoHipError(f"frame_metrics: {name} must be on the GPU (cuda device); there is no CPU "
                                     "fallback")
    dev = pred.device
    if real.device != dev:
        raise ValueError(f"frame_metrics: pred on {dev}, real on {real.device}")
    out = {}
    if "lpips" in metrics:
        with torch.no_grad():
            d = lpips(_unit_frames(pred, lo, hi, quantize) * 2.0 - 1.0, _unit_frames(real, lo, hi, quantize) * 2.0 - 1.0)
        out["lpips"] = d.float().view(b, t)
        if not mask:
            return out
    part_bytes = _lib.query("waldo_frame_metrics_partial_bytes", b, t, h, w, mask)
    scratch_bytes = _lib.query("waldo_frame_metrics_scratch_bytes", b, t, h, w, mask)
    if part_bytes < 0 or scratch_bytes < 0:
        raise ValueError(f"frame_metrics: unsupported shape {shp}")
    da, ea, sa = _descriptor(pred)
    db, eb, sb = _descriptor(real)
    partials = torch.empty(max(part_bytes // 8, 1), dtype=torch.float64, device=dev)
    scratch = torch.empty(scratch_bytes // 4, dtype=torch.float32, device=dev) if scratch_bytes else None
    out.update({m: torch.empty(b, t, dtype=torch.float32, device=dev) for m in metrics if m in _BITS})
    table = rgb_table(dev) if _ENC_PACKED in (ea, eb) else None
    _lib.launch("waldo_frame_metrics_fwd", dev, da, ea, *sa, db, eb, *sb, table, b, t, h, w, lo, hi - lo,
                QUANTIZE[quantize], mask, partials, scratch, out.get("psnr"), out.get("ssim"), out.get("msssim"))
    return {m: out[m] for m in metrics}


def summarize(scores, vid_context):
    """The reference's aggregation (tools/eval/metrics.py:95-113) of per-frame scores: ``scores`` maps a metric name
    to a (clips, T) array (a tensor from ``frame_metrics``, or stacked batches of them).  Returns a plain dict::

        {name: {"per_t": [{"t": t, "mean": m, "std": s}, ...],            # over clips, np.std (ddof 0)
                "cum": [{"t": t, "mean": m, "std": s}, ...]}}             # clips x frames vid_context..t, t >= vid_context

    that ``json.dump`` writes as it is."""
    out = {}
    for name, v in scores.items():
        a = v.detach().cpu().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError(f"summarize: {name} must be (clips, T), got shape {a.shape}")
        with np.errstate(invalid="ignore"):  # PSNR +inf (frames equal to the real ones): np.std gives nan, as there
            per_t = [{"t": t, "mean": float(np.mean(a[:, t])), "std": float(np.std(a[:, t]))} for t in range(a.shape[1])]
            cum = [{"t": t, "mean": float(np.mean(a[:, vid_context:t + 1])),
                    "std": float(np.std(a[:, vid_context:t + 1]))} for t in range(vid_context, a.shape[1])]
        out[name] = {"per_t": per_t, "cum": cum}
    return out


def format_lines(summary):
    """The reference's closing lines (metrics.py:109-113): ``[name:t] : (mean, std)`` for every t and metric, and
    ``[cum name:t] : (mean, std)`` from the context length on."""
    lines = []
    names = list(summary)
    n_t = len(summary[names[0]]["per_t"]) if names else 0
    for t in range(n_t):
        for name in names:
            p = summary[name]["per_t"][t]
            lines.append(f"[{name}:{t}] : {(p['mean'], p['std'])}")
            cum = {c["t"]: c for c in summary[name]["cum"]}
            if t in cum:
                lines.append(f"[cum {name}:{t}] : {(cum[t]['mean'], cum[t]['std'])}")
    return lines
