"""What the supervision kernels compute (waldo_amd/csrc/supervision.hip), restated in plain torch in fp32 with the
kernels' geometry and one named FAULT at a time: the candidates that test_supervision_sensitivity_cpu.py hands to the
check helpers of tests/test_gpu_supervision.py in place of the kernels.

``cell_distance``: per frame and chunk of kCellChunk pixels a partial at ``f * chunks + c``, the chosen object per pixel
as a byte, one finishing pass over the partials; backward per chunk the sums of (-2 w gx, -2 w gy, w) per chosen object
and grad_fg, then the moments' gradient summed over a frame's chunks.  The poses reach the moments through
``supervision.cell_moments`` and autograd, as in the wrapper.

``gaussian_blur``: per 32 x 64 tile the input with its k / 2 halo (rows and columns reflected at the IMAGE's border,
read from the neighbouring tile elsewhere), the row pass into a second buffer, the column pass out of it; the weights as
the host computes them, in fp32."""
import numpy as np
import torch

import supervision_ref as R

BLOCK, CELL_CHUNK, CELL_MAX_OBJ = 256, 2048, 31   # kBlock, kCellChunk, kCellMaxObj
BLUR_TH, BLUR_TW, BLUR_MAX_K = 32, 64, 31         # kBlurTH, kBlurTW, kBlurMaxK

CELL_FAULTS = {
    "last_chunk_dropped": "chunks = HW / kCellChunk rounded DOWN (at least 1): a ragged last chunk after the first is "
                          "never launched nor summed",
    "partials_indexed_chunk_major": "the backward writes its partial at c * F + f; the moments gradient reads "
                                    "f * chunks + c",
    "mean_stops_at_256_partials": "the finishing pass reads one partial per thread: no stride loop",
    "chosen_read_from_chunk_0": "the backward reads the chosen object at the chunk-local pixel index",
    "tail_lanes_live": "no bound test: the lanes past H W of the last chunk are counted at the clamped index H W - 1",
    "object_30_unreachable": "the minimum stops at 30 objects",
    "bound_on_chunk_local_index": "the bound is tested on the chunk-local index: only in a LATER chunk are the lanes "
                                  "past H W counted (at H W - 1) -- the variant of tail_lanes_live one chunk cannot show",
}
BLUR_FAULTS = {
    "tile_row_halo_reflected_at_tile": "the halo rows are mirrored at the tile's first / last row instead of read from "
                                       "the neighbouring tile",
    "column_pass_shifted_in_second_tile_row": "from the second tile row on the column pass starts one row late",
    "taps_beyond_23_dropped": "rows and columns stop after 23 taps",
}


# ---------------------------------------------------------------------------------------------------------------------
# cell distance
# ---------------------------------------------------------------------------------------------------------------------
def _chunks(hw, fault):
    full = -(-hw // CELL_CHUNK)
    return full, (max(1, hw // CELL_CHUNK) if fault == "last_chunk_dropped" else full)


def _chunk_pixels(c, hw, w, gx, gy, k, fault):
    """The live lanes of chunk ``c``: (pixel index, px, py, kg2)."""
    local = torch.arange(CELL_CHUNK)
    i = c * CELL_CHUNK + local
    if fault == "tail_lanes_live":
        live = torch.ones_like(local, dtype=torch.bool)
    else:
        live = (local if fault == "bound_on_chunk_local_index" else i) < hw
    i = i[live].clamp_max(hw - 1)
    y = i // w
    px, py = gx[i - y * w], gy[y]
    return i, px, py, k * (px * px + py * py)


def _weights(mask, fg, i, eps):
    return mask[:, i] if fg is None else (mask[:, i] + eps) * (1.0 - fg[:, i])


def _dis(px, py, kg2, mom):
    """(kg2 - 2 (px S1x + py S1y)) + S2 per (frame, object, pixel): the kernels' one definition."""
    return (kg2 - 2.0 * (px * mom[:, :, 0:1] + py * mom[:, :, 1:2])) + mom[:, :, 2:3]


def cell_term(mom, mask, fg, gx, gy, k, eps, fault=None):
    """One launch pair forward and one backward (grad_out = 1): mom (F, No, 3), mask and fg (F, H W), fg None for the
    centre term.  Returns (value, grad_moments (F, No, 3), grad_fg (F, H W) or None)."""
    nf, no = mom.shape[:2]
    hw, w = mask.shape[1], gx.numel()
    full, chunks = _chunks(hw, fault)
    count = torch.tensor(float(nf) * hw, dtype=torch.float32)
    reach = min(no, 30) if fault == "object_30_unreachable" else no
    frames = torch.arange(nf)
    # forward
    partial = torch.zeros(nf * full)
    chosen = torch.full((nf, hw), 255, dtype=torch.uint8)
    for c in range(chunks):
        i, px, py, kg2 = _chunk_pixels(c, hw, w, gx, gy, k, fault)
        v = _weights(mask, fg, i, eps)[:, None] * _dis(px, py, kg2, mom)
        best = v[:, :reach].min(dim=1)
        chosen[:, i] = best.indices.to(torch.uint8)
        partial[frames * chunks + c] = best.values.sum(dim=1)
    if fault == "mean_stops_at_256_partials":
        partial = partial[:BLOCK]
    value = partial.sum() / count
    # backward
    scale = torch.tensor(1.0) / count
    parts = torch.zeros(nf * full, no, 3)
    grad_fg = None if fg is None else torch.zeros_like(fg)
    for c in range(chunks):
        i, px, py, kg2 = _chunk_pixels(c, hw, w, gx, gy, k, fault)
        wgt = _weights(mask, fg, i, eps)
        read = (i - c * CELL_CHUNK).clamp_min(0) if fault == "chosen_read_from_chunk_0" else i
        idx = chosen[:, read].long()
        if grad_fg is not None:
            d = _dis(px, py, kg2, mom).gather(1, idx.clamp_max(no - 1)[:, None])[:, 0]
            grad_fg[:, i] = -(scale * ((mask[:, i] + eps) * d))
        hot = torch.nn.functional.one_hot(idx.clamp_max(no), no + 1)[:, :, :no].float()     # (F, px, No); 255: none
        sums = torch.stack([-2.0 * (wgt * px), -2.0 * (wgt * py), wgt], dim=-1)             # (F, px, 3)
        slot = c * nf + frames if fault == "partials_indexed_chunk_major" else frames * chunks + c
        parts[slot] = torch.einsum("fpn,fpj->fnj", hot, sums)
    grad_mom = torch.zeros_like(mom)
    for c in range(chunks):
        grad_mom += parts[frames * chunks + c]
    return value, scale * grad_mom, grad_fg


def cell_distance(fault=None):
    """``fn(pose, fg, mask, obj_shape, eps, center=True)`` -> (cell_dis, center_dis, grad pose, grad fg_mask, grad pose
    of center_dis), the tuple the GPU tests take from the wrapper and autograd."""
    from waldo_amd.supervision import cell_moments
    from waldo_amd.tools.utils import get_grid
    assert fault is None or fault in CELL_FAULTS, fault   # (an unknown name would run as no fault at all)

    def fn(pose, fg, mask, obj_shape, eps, center=True):
        h, w = mask.shape[-2:]
        g = get_grid(h, w)
        gx, gy = g[0, 0, :, 0].contiguous(), g[0, :, 0, 1].contiguous()
        p = pose.clone().requires_grad_()
        cell, centre = cell_moments(p, obj_shape)
        no = pose.shape[2]
        flat = lambda x: x.reshape(-1, h * w)  # noqa: E731
        k = float((obj_shape[0] - 1) * (obj_shape[1] - 1))
        with torch.no_grad():
            val, gm, gf = cell_term(cell.detach().reshape(-1, no, 3), flat(mask), flat(fg), gx, gy, k, float(eps), fault)
        gp, = torch.autograd.grad(cell, [p], gm.view_as(cell), retain_graph=True)
        if not center:
            return val, None, gp, gf.view_as(fg), None
        with torch.no_grad():
            cval, cgm, _ = cell_term(centre.detach().reshape(-1, no, 3), flat(mask), None, gx, gy, 1.0, 0.0, fault)
        gpc, = torch.autograd.grad(centre, [p], cgm.view_as(centre))
        return val, cval, gp, gf.view_as(fg), gpc

    return fn


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian blur
# ---------------------------------------------------------------------------------------------------------------------
def blur_weights(k, sigma):
    """The host's weights: exp(-0.5 q^2) at q = (i - k / 2) / sigma in fp32, summed in order, divided."""
    f = np.float32
    q = (np.arange(k) - k // 2).astype(f) / f(sigma)
    wt = np.exp(f(-0.5) * (q * q)).astype(f)
    total = f(0)
    for v in wt:
        total = f(total + v)
    return torch.from_numpy((wt / total).astype(f))


def _reflect_clamped(i, lo, hi):
    """Reflection without the border pixel about [lo, hi], then the clamp (csrc: reflect_clamped, there lo = 0)."""
    i = torch.where(i < lo, 2 * lo - i, i)
    i = torch.where(i > hi, 2 * hi - i, i)
    return i.clamp(lo, hi)


def gaussian_blur(fault=None):
    """``fn(x, sigma, k)`` on (..., H, W) fp32."""
    assert fault is None or fault in BLUR_FAULTS, fault

    def fn(x, sigma, k=23):
        h, w = x.shape[-2:]
        planes = x.reshape(-1, h, w)
        out = torch.empty_like(planes)
        wt = blur_weights(k, sigma)
        p = k // 2
        taps = min(k, 23) if fault == "taps_beyond_23_dropped" else k
        for y0 in range(0, h, BLUR_TH):
            for x0 in range(0, w, BLUR_TW):
                rows = torch.arange(y0 - p, y0 + BLUR_TH + p)
                if fault == "tile_row_halo_reflected_at_tile":
                    rows = _reflect_clamped(rows, y0, min(y0 + BLUR_TH, h) - 1)
                rows = _reflect_clamped(rows, 0, h - 1)
                cols = _reflect_clamped(torch.arange(x0 - p, x0 + BLUR_TW + p), 0, w - 1)
                tile = planes[:, rows][:, :, cols]                                    # (P, TH + 2p, TW + 2p)
                mid = torch.zeros(planes.shape[0], BLUR_TH + 2 * p, BLUR_TW)
                for j in range(taps):
                    mid = mid + wt[j] * tile[:, :, j:j + BLUR_TW]
                late = 1 if fault == "column_pass_shifted_in_second_tile_row" and y0 > 0 else 0
                acc = torch.zeros(planes.shape[0], BLUR_TH, BLUR_TW)
                for d in range(taps):
                    r = (torch.arange(BLUR_TH) + d + late).clamp_max(BLUR_TH + 2 * p - 1)
                    acc = acc + wt[d] * mid[:, r]
                th, tw = min(BLUR_TH, h - y0), min(BLUR_TW, w - x0)
                out[:, y0:y0 + th, x0:x0 + tw] = acc[:, :th, :tw]
        return out.view_as(x)

    return fn


def moving_object_target(fault=None):
    """``fn(flow, lyt, fg, bg, other, **options)``: the restatement of the target in fp32 with the blur above in
    place of its own -- the blur is the one tiled kernel of the target that the edge tests do not already cover."""
    from waldo_amd.supervision import MovingObjectTarget
    blur = gaussian_blur(fault)

    def fn(flow, lyt, fg, bg, other, **options):
        keep = R.gaussian_blur
        R.gaussian_blur = lambda x, sigma, k=23: blur(x, sigma, k)
        try:
            r = R.moving_object_target(flow, lyt, fg, bg, other, **options)
        finally:
            R.gaussian_blur = keep
        return MovingObjectTarget(*(r[name] for name in MovingObjectTarget._fields))

    return fn
