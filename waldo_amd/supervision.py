"""Moving-object supervision for LVD training, made on the device (include/waldo_hip.h "Supervision targets"): the
target ``Synthesizer.extract_object`` builds from the real flow and layout on every step (models/synthesizer.py:907-945;
models/modules/edge.py), the control-point distance terms (synthesizer.py:965-979) without their
(B, T, No, cells, H, W) tensor, and the recipe's four-term objective on top (scripts/cityscapes/train_lvd.sh:15).

    edge, dominant = flow_edges(real_flow, 15)                        # EdgeExtractor.forward, one launch
    y = gaussian_blur(x, sigma=2.0)                                    # the reference's blur(), one launch
    tgt = moving_object_target(real_flow, real_lyt, fg, bg, other, flow_thresh=0.02, mov_obj_thresh=0.005,
                               blur_sigma=2.0, edge_size=15, use_fg=True, use_dominant_flow_other=True)
    loss = cell_distance(obj_pose, (4, 4), tgt.mov_obj_mask, fg_mask)  # autograd: to the poses and to fg_mask
    terms = recipe_terms(alpha_flt, rec_flow, real_flow, real_lyt, obj_pose, (4, 4), tgt)

fp32, contiguous NCHW.  The target carries no gradient; ``cell_distance`` sums without float atomics, so its value and
gradients are the same bits from run to run in either mode of ``set_deterministic``.  No CPU fallback.

Below them the objective of the future layer predictor's step (synthesizer.py:752-754), the one entry here that also
serves CPU tensors and other dtypes, in framework ops:

    terms = pose_terms((real_obj_pose, real_bg_pose, real_occ_score), (pred_obj_pose, pred_bg_pose, pred_occ_score), ctx_mask)"""
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import _lib
from .tools.utils import get_grid

EDGE_MAX_KERNEL, BLUR_MAX_KERNEL = 15, 31
MAX_LAYOUT_CHANNELS, MAX_OBJECTS = 32, 31
_FLAGS = {"use_fg": 1, "use_nobg": 2, "use_nobg_edge": 4, "use_flow_nobg": 8, "use_dominant_flow_other": 16}  # WALDO_MOV_*


class MovingObjectTarget(NamedTuple):
    """``moving_object_target``'s result, every field (..., C, H, W) with the inputs' leading dimensions."""
    mov_obj_mask: torch.Tensor   # C = 1: delta_flow > mov_obj_thresh and the optional branches (synthesizer.py:922-930)
    mov_obj: torch.Tensor        # C = 1: 2 mask - 1, reg_bg_mul on the negatives, the masked overwrites (:934-942)
    fg_prop: torch.Tensor        # C = 1 (:912)
    mean_bg_flow: torch.Tensor   # C = 2 (:916-919)
    flow_edge: torch.Tensor      # C = 1: the thresholded 0 / 1 map (:909)
    dominant_flow: torch.Tensor  # C = 1: 0 / 1 (edge.py:35)


def _check(fn, x, what, channels=None):
    """``x`` must be (..., C, H, W) fp32 data: no gradient."""
    if not torch.is_tensor(x) or x.ndim < 3 or x.dtype != torch.float32:
        raise ValueError(f"{fn}: {what} must be a (..., C, H, W) float32 tensor, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if channels is not None and x.shape[-3] != channels:
        raise ValueError(f"{fn}: {what} must have {channels} channels, got {tuple(x.shape)}")
    if x.requires_grad:
        raise ValueError(f"{fn}: {what} requires grad; the target is data and has no backward (detach it)")


def _frames(fn, x, what):
    """A checked ``x`` as contiguous (N, C, H, W) on the GPU, and its leading shape."""
    if not x.is_cuda:
        raise _lib.WaldoHipError(f"{fn}: {what} must be on the GPU (cuda device); there is no CPU fallback")
    return x.contiguous().view(-1, *x.shape[-3:]), tuple(x.shape[:-3])


def _odd(fn, k, max_k, h, w):
    k = int(k)
    if k < 3 or k > max_k or k % 2 == 0:
        raise ValueError(f"{fn}: kernel_size must be odd and in [3, {max_k}], got {k}")
    if h <= k // 2 or w <= k // 2:
        raise ValueError(f"{fn}: H, W = {h}, {w} must exceed the reflection padding {k // 2}")
    return k


def _flow_edges(fn, flow, k, eps):
    n, c, h, w = flow.shape
    k = _odd(fn, k, EDGE_MAX_KERNEL, h, w)
    edge, dominant = flow.new_empty(n, 1, h, w), flow.new_empty(n, 1, h, w)
    _lib.launch("waldo_flow_edges_fwd", flow.device, flow, edge, dominant, n, c, h, w, k, float(eps))
    return edge, dominant


def _blur(fn, x, sigma, k):
    n, c, h, w = x.shape
    k = _odd(fn, k, BLUR_MAX_KERNEL, h, w)
    sigma = float(sigma)
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"{fn}: sigma must be positive and finite, got {sigma}")
    y = torch.empty_like(x)
    _lib.launch("waldo_gaussian_blur_fwd", x.device, x, y, n * c, h, w, k, sigma)
    return y


def flow_edges(flow, kernel_size=15, eps=1e-6):
    """``EdgeExtractor(kernel_size).forward(flow, eps)`` (models/modules/edge.py:28-40) in one launch: ``flow``
    (B, T, 2, H, W) or (N, 2, H, W) -> ``(flow_edge, dominant_flow)``, one channel each.  Reflection padding k // 2; per
    channel the k x k mean and the two gradient filters ``x_i / (x_i^2 + y_j^2)``, ``y_j / (x_i^2 + y_j^2)``;
    ``flow_edge = 1 - prod_c (1 - sqrt(gx^2 + gy^2 + eps) / sqrt(32))``; ``dominant_flow`` is 1.0 where the flow's squared
    norm exceeds its local mean's.  ``kernel_size`` odd in [3, 15]; H, W > kernel_size // 2."""
    _check("flow_edges", flow, "flow", channels=2)
    d, lead = _frames("flow_edges", flow, "flow")
    edge, dominant = _flow_edges("flow_edges", d, kernel_size, eps)
    h, w = d.shape[-2:]
    return edge.view(*lead, 1, h, w), dominant.view(*lead, 1, h, w)


def gaussian_blur(x, sigma, kernel_size=23):
    """The reference's ``blur`` (models/synthesizer.py:1114-1118: ``GaussianBlur(kernel_size, sigma)`` with a fixed
    sigma) of ``x`` (..., C, H, W), depthwise, in one launch: 1-D weights ``exp(-(t / sigma)^2 / 2)`` at
    ``t = linspace(-(k - 1) / 2, (k - 1) / 2, k)`` normalised to sum 1, rows then columns, reflection padding k // 2.
    ``kernel_size`` odd in [3, 31]; H, W > kernel_size // 2."""
    _check("gaussian_blur", x, "x")
    d, lead = _frames("gaussian_blur", x, "x")
    return _blur("gaussian_blur", d, sigma, kernel_size).view(*lead, *d.shape[-3:])


def _bits(fn, idx, nl, what):
    bits = 0
    for i in idx:
        i = int(i)
        if not 0 <= i < nl:
            raise ValueError(f"{fn}: {what} names the channel {i}, the layout has {nl}")
        bits |= 1 << i
    return bits


def moving_object_target(real_flow, real_lyt, fg_idx, bg_idx, other_idx, *, flow_thresh, mov_obj_thresh, blur_sigma,
                         edge_size, reg_bg_mul=0.25, use_fg=False, use_nobg=False, use_nobg_edge=False,
                         nobg_edge_mul=0.0, use_flow_nobg=False, use_dominant_flow_other=False):
    """The moving-object target of models/synthesizer.py:907-942 (``blur_alpha`` off) from the real flow (..., 2, H, W)
    and layout (..., Nl, H, W): four launches -- the flow edges, the sums over the three channel lists, the blur of
    ``(1 - fg_prop) * (1, flow)`` (kernel size 23) and the thresholds / masked overwrites.  The keyword names are the
    reference's options.  Returns a ``MovingObjectTarget``; nothing carries a gradient and an input that requires one is
    refused.  ``use_flow_nobg`` with ``use_dominant_flow_other`` is refused: the reference's ``|`` of a float mask raises."""
    fn = "moving_object_target"
    _check(fn, real_flow, "real_flow", channels=2)
    _check(fn, real_lyt, "real_lyt")
    nl, h, w = real_lyt.shape[-3:]
    if real_lyt.shape[:-3] != real_flow.shape[:-3] or tuple(real_flow.shape[-2:]) != (h, w):
        raise ValueError(f"{fn}: real_flow {tuple(real_flow.shape)} and real_lyt {tuple(real_lyt.shape)} disagree")
    if nl > MAX_LAYOUT_CHANNELS:
        raise ValueError(f"{fn}: {nl} layout channels (at most {MAX_LAYOUT_CHANNELS}: the lists travel as bit masks)")
    if use_flow_nobg and use_dominant_flow_other:
        raise ValueError(f"{fn}: use_flow_nobg with use_dominant_flow_other (the reference raises on that pair)")
    fg, bg, other = (_bits(fn, idx, nl, name) for idx, name in ((fg_idx, "fg_idx"), (bg_idx, "bg_idx"),
                                                                 (other_idx, "other_idx")))
    opts = dict(use_fg=use_fg, use_nobg=use_nobg, use_nobg_edge=use_nobg_edge, use_flow_nobg=use_flow_nobg,
                use_dominant_flow_other=use_dominant_flow_other)
    flags = sum(bit for name, bit in _FLAGS.items() if opts[name])
    flow, lead = _frames(fn, real_flow, "real_flow")
    lyt, _ = _frames(fn, real_lyt, "real_lyt")
    n = lyt.shape[0]
    edge_raw, dominant = _flow_edges(fn, flow, edge_size, 1e-6)
    props = flow.new_empty(3, n, 1, h, w)
    blur_in = flow.new_empty(n, 3, h, w)
    _lib.launch("waldo_mov_props_fwd", flow.device, lyt, flow, fg, bg, other, props[0], props[1], props[2], blur_in, n, nl,
                h * w)
    blurred = _blur(fn, blur_in, blur_sigma, 23)
    out = flow.new_empty(3, n, 1, h, w)
    mean_bg_flow = flow.new_empty(n, 2, h, w)
    _lib.launch("waldo_mov_finish_fwd", flow.device, flow, blurred, props[0], props[1], props[2], edge_raw, dominant,
                float(flow_thresh), float(mov_obj_thresh), float(reg_bg_mul), float(nobg_edge_mul), flags, out[0],
                mean_bg_flow, out[1], out[2], n, h * w)
    one = (*lead, 1, h, w)
    return MovingObjectTarget(mov_obj_mask=out[1].view(one), mov_obj=out[2].view(one), fg_prop=props[0].view(one),
                              mean_bg_flow=mean_bg_flow.view(*lead, 2, h, w), flow_edge=out[0].view(one),
                              dominant_flow=dominant.view(one))


# --------------------------------------------------------------------------------------
# control-point distances
# --------------------------------------------------------------------------------------
_grids = {}


def _pixel_axes(h, w, device):
    """The columns (W) and rows (H) of ``get_grid(H, W)`` (``warper.src_grid``) on ``device``, made once."""
    key = (h, w, str(device))
    if key not in _grids:
        g = get_grid(h, w)
        _grids[key] = (g[0, 0, :, 0].contiguous().to(device), g[0, :, 0, 1].contiguous().to(device))
    return _grids[key]


def cell_moments(obj_pose, obj_shape):
    """The moments the distance kernels read, in framework ops (autograd carries their gradient to the poses):
    ``obj_pose`` (B, T, No, ho * wo, 2) -> ``(cell, center)``, each (B, T, No, 3) = (sum c_x, sum c_y, sum |c|^2) over the
    object's (ho - 1)(wo - 1) cell centres (synthesizer.py:967-968) and over its one centre (:969)."""
    ho, wo = (int(v) for v in obj_shape)
    g = obj_pose.reshape(*obj_pose.shape[:3], ho, wo, 2)
    cell = (g[:, :, :, 1:, 1:] + g[:, :, :, 1:, :-1] + g[:, :, :, :-1, 1:] + g[:, :, :, :-1, :-1]) / 4
    cell = cell.reshape(*obj_pose.shape[:3], -1, 2)
    center = obj_pose.mean(dim=3)
    return (torch.cat([cell.sum(dim=3), (cell ** 2).sum(dim=(3, 4)).unsqueeze(-1)], dim=-1),
            torch.cat([center, (center ** 2).sum(dim=-1, keepdim=True)], dim=-1))


class _CellDistance(torch.autograd.Function):
    """mean over pixels of min over objects of w * (K |g|^2 - 2 g . S1 + S2): the value, the chosen object per pixel as a
    byte for the backward.  ``fg_mask`` None: w = mov_mask (the centre term); else w = (mov_mask + eps)(1 - fg_mask)."""

    @staticmethod
    def forward(ctx, moments, fg_mask, mov_mask, k, eps):
        f, no = moments.shape[0] * moments.shape[1], moments.shape[2]
        h, w = mov_mask.shape[-2:]
        dev = moments.device
        moments = moments.contiguous()
        fg = None if fg_mask is None else fg_mask.contiguous()
        gx, gy = _pixel_axes(h, w, dev)
        out = moments.new_empty(1)
        chosen = torch.empty(f, h, w, dtype=torch.uint8, device=dev)
        nbytes = _lib.query("waldo_cell_distance_workspace_bytes", f, no, h * w)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.launch("waldo_cell_distance_fwd", dev, moments, mov_mask, fg, gx, gy, out, chosen, ws, nbytes, f, no, h, w,
                    float(k), float(eps))
        ctx.save_for_backward(moments, fg, mov_mask, chosen)
        ctx.args = (f, no, h, w, float(k), float(eps), nbytes)
        return out.view(())

    @staticmethod
    def backward(ctx, grad_out):
        moments, fg, mov_mask, chosen = ctx.saved_tensors
        f, no, h, w, k, eps, nbytes = ctx.args
        dev = moments.device
        gx, gy = _pixel_axes(h, w, dev)
        grad_moments = torch.empty_like(moments)
        grad_fg = torch.empty_like(fg) if fg is not None and ctx.needs_input_grad[1] else None
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.launch("waldo_cell_distance_bwd", dev, moments, mov_mask, fg, gx, gy, chosen, grad_out.contiguous(),
                    grad_moments, grad_fg, ws, nbytes, f, no, h, w, k, eps)
        return grad_moments, grad_fg, None, None, None


def cell_distance(obj_pose, obj_shape, mov_obj_mask, fg_mask, eps=0.0, center=False):
    """``cell_dis`` of models/synthesizer.py:965-977 -- ``((mov_obj_mask + eps) * (1 - fg_mask) * obj_cell_dis).min(dim=2)
    [0].mean()`` -- without the (B, T, No, cells, H, W) tensor: the sum over an object's cells is analytic in the cells'
    moments (``cell_moments``), and one pass takes the minimum over the objects per pixel.  ``obj_pose``
    (B, T, No, ho * wo, 2) with ``obj_shape = (ho, wo)``, ho, wo >= 2, No <= 31; the masks (B, T, 1, H, W); the pixel
    coordinates are ``get_grid(H, W)``.  With ``center`` also ``center_dis`` (:973-979), returned second.  Gradients reach
    ``obj_pose`` and ``fg_mask``; ``mov_obj_mask`` is a constant.  Ties go to the lowest object index (``torch.min`` on the
    CPU).  No float atomics: the same bits from run to run, whatever ``set_deterministic`` says."""
    fn = "cell_distance"
    ho, wo = (int(v) for v in obj_shape)
    if ho < 2 or wo < 2:
        raise ValueError(f"{fn}: obj_shape {tuple(obj_shape)} has no cell (ho, wo >= 2)")
    if obj_pose.ndim != 5 or obj_pose.shape[3] != ho * wo or obj_pose.shape[4] != 2 or obj_pose.dtype != torch.float32:
        raise ValueError(f"{fn}: obj_pose must be float32 (B, T, No, {ho * wo}, 2), got {obj_pose.dtype} "
                         f"{tuple(obj_pose.shape)}")
    b, t, no = obj_pose.shape[:3]
    if not 1 <= no <= MAX_OBJECTS:
        raise ValueError(f"{fn}: No = {no} objects outside [1, {MAX_OBJECTS}]")
    for name, m in (("mov_obj_mask", mov_obj_mask), ("fg_mask", fg_mask)):
        if m.ndim != 5 or tuple(m.shape[:3]) != (b, t, 1) or m.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} must be float32 ({b}, {t}, 1, H, W), got {m.dtype} {tuple(m.shape)}")
    if mov_obj_mask.shape != fg_mask.shape:
        raise ValueError(f"{fn}: mov_obj_mask {tuple(mov_obj_mask.shape)} and fg_mask {tuple(fg_mask.shape)} disagree")
    if mov_obj_mask.requires_grad:
        raise ValueError(f"{fn}: mov_obj_mask requires grad; it is a constant of the objective (detach it)")
    for name, x in (("obj_pose", obj_pose), ("mov_obj_mask", mov_obj_mask), ("fg_mask", fg_mask)):
        if not x.is_cuda:
            raise _lib.WaldoHipError(f"{fn}: {name} must be on the GPU (cuda device); there is no CPU fallback")
    cell, centre = cell_moments(obj_pose, (ho, wo))
    m = mov_obj_mask.contiguous()
    cell_dis = _CellDistance.apply(cell, fg_mask, m, (ho - 1) * (wo - 1), eps)
    if not center:
        return cell_dis
    return cell_dis, _CellDistance.apply(centre, None, m, 1, 0.0)


def recipe_terms(alpha_flt, rec_flow, real_flow, real_lyt, obj_pose, obj_shape, target, *, cell_dis_eps=0.0):
    """The four terms of the reference's LVD recipe (``--s_vid_object_extractor_losses "ent_flt_edge" "l1_flow"
    "cell_dis" "reg_mov"``) as a dict of scalars.  ``alpha_flt`` (B, T, No + 1, H, W) the filtered composited alphas in
    [-1, 1] (``swap_flt``: they stand for ``rec_output_alpha``), ``rec_flow`` (B, T - 1, 2, H, W), ``target`` a
    ``MovingObjectTarget``.  ``cell_dis`` is ``cell_distance`` with ``fg_mask = sum_obj (alpha_flt + 1) / 2``
    (synthesizer.py:931); the other three are plain framework ops: ``reg_mov`` (:951), ``ent_flt_edge`` (:888-899, its
    edge mask through ``gaussian_blur(.., 2, 3)``), ``l1_flow`` (:989)."""
    fg_mask = ((alpha_flt[:, :, 1:] + 1) / 2).sum(dim=2, keepdim=True)
    cell_dis = cell_distance(obj_pose, obj_shape, target.mov_obj_mask, fg_mask, eps=cell_dis_eps)
    reg_mov = (target.mov_obj * -fg_mask).mean()
    ent = F.normalize((alpha_flt + 1) / 2 + 1e-6, p=1, dim=2)
    ent = -torch.sum(ent * torch.log(ent + 1e-6), dim=2, keepdim=True) / 0.37
    lyt_edge_mask = (gaussian_blur(real_lyt / 10 + 1 / 2, 2.0, 3).amax(dim=2, keepdim=True) > 0.999).float()
    return {"cell_dis": cell_dis, "reg_mov": reg_mov, "ent_flt_edge": (ent * lyt_edge_mask).mean(),
            "l1_flow": (real_flow[:, 1:] - rec_flow).abs().mean()}


# --------------------------------------------------------------------------------------
# the pose objective of the future layer predictor's step
# --------------------------------------------------------------------------------------
POSE_TERMS = ("rec_obj_pose", "rec_bg_pose", "rec_occ_score")  # synthesizer.py:752-754


def _pose_mask(fn, ctx_mask, batch, steps, device):
    """``ctx_mask`` as a contiguous (B, T) tensor of one byte per frame on ``device``, non-zero = context frame.  A plan's
    bytes are scattered once from its frame indices, on the device and without a host read, and kept on the plan."""
    from .modules.transform import ClipPlan
    from .nets.flp import FlpPlan
    plan = ctx_mask.frames if isinstance(ctx_mask, FlpPlan) else ctx_mask  # (the ClipPlan of the mask itself)
    if isinstance(plan, ClipPlan):
        mask = getattr(plan, "_pose_mask", None)
        if mask is None:
            mask = torch.zeros(plan.batch * plan.steps, dtype=torch.uint8, device=plan.index.device)
            mask = plan._pose_mask = mask.index_fill_(0, plan.index, 1).view(plan.batch, plan.steps)
        what = f"the plan's mask uint8 {tuple(mask.shape)}"
    else:
        mask = ctx_mask
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.ndim != 2:
            raise ValueError(f"{fn}: ctx_mask must be a boolean (B, T) tensor or a plan, got "
                             f"{getattr(mask, 'dtype', type(mask).__name__)} {tuple(getattr(mask, 'shape', ()))}")
        what = f"ctx_mask bool {tuple(mask.shape)}"
    if tuple(mask.shape) != (batch, steps):
        raise ValueError(f"{fn}: {what} does not cover the poses' ({batch}, {steps}) frames")
    if mask.device != device:
        raise ValueError(f"{fn}: {what} is on {mask.device}, the poses are on {device}")
    return mask.contiguous()


class _PoseL1(torch.autograd.Function):
    """The three masked L1 means in one forward call and one backward launch; ``kept``, the number of kept frames, stays
    on the device between the two."""

    @staticmethod
    def forward(ctx, mask, *pairs):
        pairs = tuple(x.contiguous() for x in pairs)   # (real, pred) x (obj, bg, occ)
        dev = pairs[0].device
        f = mask.numel()
        sizes = tuple(x.numel() // f for x in pairs[::2])
        out = torch.empty(4, dtype=torch.float32, device=dev)  # the three terms, kept
        nbytes = _lib.query("waldo_pose_l1_workspace_bytes", f, *sizes)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.launch("waldo_pose_l1_fwd", dev, *pairs, mask, out, out[3:], ws, nbytes, f, *sizes)
        ctx.save_for_backward(mask, out, *pairs)
        ctx.sizes = (f, *sizes)
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, *grads):
        mask, out, *pairs = ctx.saved_tensors
        grads = [None if g is None else g.contiguous() for g in grads]
        grad_pred = [torch.empty_like(x) for x in pairs[1::2]]
        grad_real = [torch.empty_like(x) if ctx.needs_input_grad[1 + 2 * k] else None for k, x in enumerate(pairs[::2])]
        _lib.launch("waldo_pose_l1_bwd", mask.device, *pairs, mask, out[3:], *grads, *grad_pred, *grad_real, *ctx.sizes)
        return (None, grad_real[0], grad_pred[0], grad_real[1], grad_pred[1], grad_real[2], grad_pred[2])


def pose_terms(real, pred, ctx_mask, *, fused=True):
    """The three terms of the future layer predictor's objective (models/synthesizer.py:752-754),
    ``(to_ctx(real, ~ctx_mask) - to_ctx(pred, ~ctx_mask)).abs().mean()`` for each of ``(obj_pose, bg_pose, occ_score)``,
    as a dict of 0-d tensors ``rec_obj_pose``, ``rec_bg_pose``, ``rec_occ_score`` -- the mean of ``|real - pred|`` over
    the frames ``ctx_mask`` does NOT select, computed without gathers and without reading anything on the host (the
    reference's ``to_ctx`` reads ``any()`` and the size of a boolean index, six times).  ``real`` and ``pred`` are
    3-tuples of tensors (B, T, ...) that agree pair by pair; ``ctx_mask`` a boolean (B, T) tensor on their device, or the
    ``FlpPlan`` / ``ClipPlan`` the network ran under.  With no frame kept the terms are NaN (the reference's mean of an
    empty selection) and every gradient is exact 0.  CUDA fp32 inputs with ``fused``: one kernel call forward and one
    backward (include/waldo_hip.h "Pose objective"), no float atomics -- the same bits from run to run, and of a strided
    input and its contiguous copy; gradients reach ``pred`` and, where it asks, ``real``.  Everything else (CPU, fp64,
    16-bit, ``fused=False``): the same masked mean in framework ops."""
    fn = "pose_terms"
    if len(real) != 3 or len(pred) != 3:
        raise ValueError(f"{fn}: real and pred must be the 3-tuples (obj_pose, bg_pose, occ_score), got {len(real)} and "
                         f"{len(pred)} entries")
    lead, dev, dtype = tuple(real[0].shape[:2]), real[0].device, real[0].dtype
    for name, r, p in zip(POSE_TERMS, real, pred):
        if not torch.is_tensor(r) or not torch.is_tensor(p) or r.shape != p.shape or r.dtype != p.dtype:
            raise ValueError(f"{fn}: the {name} pair disagrees: real {getattr(r, 'dtype', type(r).__name__)} "
                             f"{tuple(getattr(r, 'shape', ()))}, pred {getattr(p, 'dtype', type(p).__name__)} "
                             f"{tuple(getattr(p, 'shape', ()))}")
        if r.ndim < 2 or tuple(r.shape[:2]) != lead or r.dtype != dtype or not r.is_floating_point():
            raise ValueError(f"{fn}: {name} must be a floating (B, T, ...) = ({lead[0]}, {lead[1]}, ...) {dtype} tensor, "
                             f"got {r.dtype} {tuple(r.shape)}")
        if r.device != dev or p.device != dev:
            raise ValueError(f"{fn}: {name} is on {r.device} / {p.device}, obj_pose is on {dev}")
        if r.numel() == 0:
            raise ValueError(f"{fn}: {name} {tuple(r.shape)} is empty")
    mask = _pose_mask(fn, ctx_mask, *lead, dev)
    if fused and dev.type == "cuda" and dtype == torch.float32:
        pairs = [x for pair in zip(real, pred) for x in pair]
        return dict(zip(POSE_TERMS, _PoseL1.apply(mask, *pairs)))
    # the masked sum, by selection: a frame that is not kept gets an exact 0 gradient whatever the count is (a product
    # with the 0 / 1 mask would hand it inf * 0 when no frame is kept)
    keep = mask == 0
    kept = keep.sum().to(dtype)
    terms = {}
    for name, r, p in zip(POSE_TERMS, real, pred):
        k = keep.view(*lead, *([1] * (r.ndim - 2)))
        terms[name] = torch.where(k, (r - p).abs(), 0).sum() / (kept * r[0, 0].numel())
    return terms
