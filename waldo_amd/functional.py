"""Autograd wrappers over the C-ABI HIP kernels (include/waldo_hip.h).

Every function here launches hand-written gfx950 kernels on the caller's current HIP stream; no
function has a CPU or eager-PyTorch fallback (``_lib.check_cuda`` raises on CPU tensors).
PyTorch is used for memory (output allocation), streams and autograd bookkeeping only.
"""
import ctypes
import math

import torch

from . import _lib


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------------------
# deterministic mode (include/waldo_hip.h "Reproducible gradients")
# --------------------------------------------------------------------------------------
_deterministic = None  # None: follow torch.are_deterministic_algorithms_enabled(); True / False: override it


def set_deterministic(mode):
    """Deterministic mode: every gradient of the library is a function of the inputs alone (the same bits from run to
    run, eagerly or replayed from a HIP graph) -- the ``*_det`` entry points replace the backward kernels that sum
    with float atomics.  ``True`` / ``False`` switch it on / off; ``None`` (the default) follows
    ``torch.are_deterministic_algorithms_enabled()``.  The mode is read when an op's FORWARD runs and travels with the
    autograd node: a graph built in one mode runs its backward in that mode.  A shape without a deterministic kernel
    raises ``WaldoHipError`` from the forward when a gradient is required."""
    global _deterministic
    if mode is not None and not isinstance(mode, bool):
        raise TypeError(f"set_deterministic: mode must be True, False or None, got {mode!r}")
    _deterministic = mode


def is_deterministic():
    """Whether an op whose forward runs now will run its backward on the deterministic kernels."""
    if _deterministic is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    return _deterministic


class deterministic:
    """``with deterministic(mode=True):`` -- ``set_deterministic(mode)`` for the block; the earlier setting comes back
    on exit, also after an exception.  Nests."""

    def __init__(self, mode=True):
        if mode is not None and not isinstance(mode, bool):
            raise TypeError(f"deterministic: mode must be True, False or None, got {mode!r}")
        self.mode = mode
        self.prev = []

    def __enter__(self):
        self.prev.append(_deterministic)
        set_deterministic(self.mode)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev.pop())
        return False


def _det_unserved(op, reason):
    return _lib.WaldoHipError(f"{op}: no deterministic kernel ({reason}); deterministic mode is on "
                              "(waldo_amd.set_deterministic / torch.use_deterministic_algorithms) and a gradient is "
                              "required")


def _det_workspace(op, query, args, device):
    """(buffer, bytes) for a ``*_det`` entry point: its ``*_det_workspace_bytes`` query, at least one word."""
    nbytes = int(_lib.query(query, *args))
    if nbytes <= 0:
        raise _det_unserved(op, f"{query}{tuple(args)} = {nbytes}")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device), nbytes


_SPLAT_MAX_CONTRIBUTIONS = 1 << 32  # per texel (include/waldo_hip.h)
_TPS_DET_MAX_K3 = 136


_MERGE_FILL_BYTES = 1 << 20


def _zeros_like_each(*tensors):
    """Zero-filled tensors shaped like each argument (None -> None), carved out of ONE buffer and filled by ONE launch:
    the gradients a backward kernel accumulates into with atomics -- at the LVD recipe a fill is a 4 us launch whatever
    its size, and a backward call that zeroed two or three small tensors paid for each.  Every view starts on a
    256-byte boundary."""
    # (only SMALL tensors share a buffer: a view keeps the whole buffer alive until every view is consumed -- a
    # full-resolution gradient tied to a tiny one that waits for another op's backward, or that AccumulateGrad keeps
    # as a leaf's .grad, would stay allocated that long)
    want = [t for t in tensors if t is not None and t.numel() * t.element_size() < _MERGE_FILL_BYTES]
    if len(want) < 2:
        return [torch.zeros_like(t) if t is not None else None for t in tensors]
    sizes = [(t.numel() + 63) // 64 * 64 for t in want]
    flat = torch.zeros(sum(sizes), dtype=want[0].dtype, device=want[0].device)
    out, at = [], 0
    it = iter(sizes)
    for t in tensors:
        if t is None:
            out.append(None)
        elif t.numel() * t.element_size() >= _MERGE_FILL_BYTES:
            out.append(torch.zeros_like(t))
        else:
            n = next(it)
            out.append(flat[at:at + t.numel()].view(t.shape))
            at += n
    return out


def _empty_like_each(*tensors):
    """Uninitialised tensors shaped like each argument (None -> None): the gradients a ``*_det`` kernel overwrites."""
    return [torch.empty_like(t) if t is not None else None for t in tensors]


class ArangeIndex(torch.Tensor):
    """A frame index KNOWN on the host to be 0, 1, ..., n - 1 (``arange_index``): ``time_gather`` may then hand out
    the clip itself instead of a gathered copy.  Plain tensors never take that short cut -- telling would need a
    device -> host read."""
    __torch_function__ = torch._C._disabled_torch_function_impl  # (results of ops on it are plain tensors)

    def __deepcopy__(self, memo):
        if _is_arange_index(self):
            return arange_index(self.numel(), self.device)
        return self.as_subclass(torch.Tensor).clone()


def arange_index(n, device=None):
    """``torch.arange(n)`` (int64) for ``pred_ts`` when every frame is predicted in order (the LVD recipe's
    ``ctx_mode "prev"``, models/synthesizer.py:833-835), marked as such: ``time_gather(x, None, pred_ts, num_ctx=1)``
    returns a VIEW of ``x`` for it (no copy forward, autograd's own sum backward) -- an alias of the caller's clip,
    unlike the reference's ``x[:, pred_ts]``; do not write to the result in place.  The mark holds for this very
    tensor while nobody writes to it (version counter).  Under HIP-graph capture the choice is frozen into the
    graph like every host-side decision."""
    t = torch.arange(int(n), device=device, dtype=torch.int64)
    if t.is_inference():  # (no version counter to vouch for it: a plain index, gathered by the kernel)
        return t
    t = t.as_subclass(ArangeIndex)
    t._waldo_arange = (int(n), t._version)
    return t


def _is_arange_index(ts):
    mark = getattr(ts, "_waldo_arange", None)
    return mark is not None and not ts.is_inference() and mark == (ts.numel(), ts._version)


def normalise_time_index(ts):
    """``ctx_ts`` / ``pred_ts`` as the kernels take them (int64, contiguous), made ONCE per decode by the
    caller (``Warper``) and handed to every op of the chain instead of converting an expanded view
    (synthesizer.py:438) into a fresh temporary per op.  No read-back: the kernels validate the indices on the
    device (``_lib.IndexStatus``)."""
    return _c(ts.long())


def _status(status):
    """(IndexStatus to hand to the kernels, whether this call checks it itself): a caller that passes its own status
    words checks them when it chooses (``Warper``: lazily, without a synchronisation); a stand-alone call uses the
    module's and is checked -- with a synchronisation -- before it returns, as the reference's ``gather`` raises."""
    return (status, False) if status is not None else (_lib.default_index_status(), True)


# --------------------------------------------------------------------------------------
# A2: TPS
# --------------------------------------------------------------------------------------
class _TpsMapping(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inverse_kernel, src_pts):
        _lib.check_cuda(inverse_kernel, src_pts)
        src_pts = _c(src_pts)
        inverse_kernel = _c(inverse_kernel)
        b, n, _ = src_pts.shape
        mapping = src_pts.new_empty(b, n + 3, 2)
        _lib.launch("waldo_tps_mapping_fwd", src_pts.device, inverse_kernel, src_pts, mapping, b, n)
        ctx.save_for_backward(inverse_kernel)
        ctx.n = n
        return mapping

    @staticmethod
    def backward(ctx, grad_mapping):
        (inverse_kernel,) = ctx.saved_tensors
        grad_mapping = _c(grad_mapping)
        b = grad_mapping.shape[0]
        grad_pts = grad_mapping.new_empty(b, ctx.n, 2)
        _lib.launch("waldo_tps_mapping_bwd", grad_mapping.device, inverse_kernel, grad_mapping, grad_pts, b, ctx.n)
        return None, grad_pts


class _TpsGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, basis_t, mapping):
        _lib.check_cuda(basis_t, mapping)
        mapping = _c(mapping)
        basis_t = _c(basis_t)
        b, k3, _ = mapping.shape
        hw = basis_t.shape[1]
        grid = mapping.new_empty(b, hw, 2)
        _lib.launch("waldo_tps_grid_fwd", mapping.device, basis_t, mapping, grid, b, hw, k3)
        ctx.save_for_backward(basis_t)
        ctx.k3 = k3
        ctx.det = is_deterministic()
        if ctx.det and ctx.needs_input_grad[1] and k3 > _TPS_DET_MAX_K3:
            raise _det_unserved("tps_grid", f"K3 = {k3} > {_TPS_DET_MAX_K3}")
        return grid

    @staticmethod
    def backward(ctx, grad_grid):
        (basis_t,) = ctx.saved_tensors
        grad_grid = _c(grad_grid)
        b, hw, _ = grad_grid.shape
        grad_mapping = grad_grid.new_empty(b, ctx.k3, 2)  # zero-filled by the launcher
        args = (basis_t, grad_grid, grad_mapping, b, hw, ctx.k3)
        if ctx.det:
            ws, nb = _det_workspace("tps_grid", "waldo_tps_grid_bwd_det_workspace_bytes", (b, hw, ctx.k3),
                                    grad_grid.device)
            _lib.launch("waldo_tps_grid_bwd_det", grad_grid.device, *args, ws, nb)
        else:
            _lib.launch("waldo_tps_grid_bwd", grad_grid.device, *args)
        return None, grad_mapping


def tps_mapping(inverse_kernel, src_pts):
    """mapping (B, N+3, 2) = K^-1 @ [src_pts; 0]  (models/modules/warp.py:52-53)."""
    return _TpsMapping.apply(inverse_kernel, src_pts.float())


def tps_grid(inverse_kernel, basis_t, src_pts, height, width):
    """TPSWarp.forward (models/modules/warp.py:49-55): (B, N, 2) -> (B, H, W, 2)."""
    mapping = tps_mapping(inverse_kernel, src_pts)
    return _TpsGrid.apply(basis_t, mapping).view(src_pts.shape[0], height, width, 2)


# --------------------------------------------------------------------------------------
# A3: grid inversion
# --------------------------------------------------------------------------------------
class _InverseWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src_grid, src_id, tgt_id, gauss, niter, erode, rank, order):
        _lib.check_cuda(src_grid, src_id, tgt_id, gauss)
        src_grid, src_id, tgt_id, gauss = _c(src_grid), _c(src_id), _c(tgt_id), _c(gauss)
        b, hs, ws, _ = src_grid.shape
        h, w = tgt_id.shape[-3], tgt_id.shape[-2]
        ksize = int(round(gauss.numel() ** 0.5))
        if ksize * ksize != gauss.numel():
            raise _lib.WaldoHipError(f"inverse_warp: a Gaussian kernel of {gauss.numel()} elements (K x K)")
        pad = niter + 1
        hwp = (h + 2 * pad) * (w + 2 * pad)
        dev = src_grid.device
        out = src_grid.new_empty(b, h, w, 2)
        dxy = src_grid.new_empty(b, 2, h * w)
        cell = torch.empty(b, h * w, dtype=torch.int32, device=dev)
        winner = torch.empty(b, h * w, dtype=torch.int32, device=dev)
        field_a = src_grid.new_empty(b, 2, hwp)
        field_b = src_grid.new_empty(b, 2, hwp)
        fill_iter = torch.empty(b, hwp, dtype=torch.uint8, device=dev)
        denom = src_grid.new_empty(b, hwp)
        mask_a = torch.empty(b, hwp, dtype=torch.uint8, device=dev)
        mask_b = torch.empty(b, hwp, dtype=torch.uint8, device=dev)
        work = (out, dxy, cell, winner, field_a, field_b, fill_iter, denom, mask_a, mask_b, b, hs, ws, h, w, niter,
                int(bool(erode)), ksize)
        if order is None:
            _lib.launch("waldo_inverse_warp_fwd", dev, src_grid, src_id, tgt_id, gauss, *work)
        else:
            if not (rank.is_cuda and order.is_cuda):
                raise _lib.WaldoHipError("inverse_warp: rank / order must be on the GPU")
            if (rank.dtype != torch.int32 or order.dtype != torch.int32
                    or rank.numel() != h * w or order.numel() != h * w):
                raise _lib.WaldoHipError("inverse_warp: rank / order must be int32 of H*W elements")
            rank, order = rank.contiguous(), order.contiguous()
            _lib.launch("waldo_inverse_warp_order_fwd", dev, src_grid, src_id, tgt_id, gauss, rank, order, *work)
        ctx.save_for_backward(gauss, cell, winner, fill_iter, denom, mask_a)
        ctx.cfg = (b, hs, ws, h, w, niter, ksize)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        gauss, cell, winner, fill_iter, denom, mask = ctx.saved_tensors
        b, hs, ws, h, w, niter, ksize = ctx.cfg
        grad_out = _c(grad_out)
        gfield = grad_out.new_empty(b, 2, fill_iter.shape[1])
        gsrc = grad_out.new_empty(b, hs, ws, 2)
        _lib.launch("waldo_inverse_warp_bwd", grad_out.device, grad_out, gauss, cell, winner, fill_iter, denom, mask,
                    gfield, gsrc, b, hs, ws, h, w, niter, ksize)
        return gsrc, None, None, None, None, None, None, None


def inverse_warp(src_grid, src_id, tgt_id, gauss, niter=5, erode=True, perm=None):
    """InverseWarp.forward (models/modules/warp.py:71-174; pad).
    src_grid (B, Hs, Ws, 2) -> (B, H, W, 2); src_id / tgt_id are the identity grids of the two
    rasters, gauss the normalised K x K Gaussian, flattened (the reference module's buffers; K odd -- 3 in every
    script: one launch each way; other sizes run the fill passes one by one).

    perm None: num_perm == 1 (the lowest sample index wins a contested cell, warp.py:113-123).
    perm (P, H*W) integer, P > 1: the reference's tie-break averaging (warp.py:91-111): for each
    row the sample standing first in that order wins, and the P elected fields are averaged.  The
    fill / erosion / crop are linear in the elected field for a fixed set of occupied cells (which
    does not depend on the order), so the average is taken over the P results instead."""
    if perm is None:
        return _InverseWarp.apply(src_grid, src_id, tgt_id, gauss, int(niter), bool(erode), None,
                                  None)
    order = perm.to(torch.int32)
    rank = torch.empty_like(order)
    pos = torch.arange(order.shape[1], dtype=torch.int32, device=order.device)
    rank.scatter_(1, order.long(), pos.expand_as(order))
    out = None
    for p in range(order.shape[0]):
        o = _InverseWarp.apply(src_grid, src_id, tgt_id, gauss, int(niter), bool(erode), rank[p],
                               order[p])
        out = o if out is None else out + o
    return out / order.shape[0]


# --------------------------------------------------------------------------------------
# A4/A5: bilinear warp
# --------------------------------------------------------------------------------------
def _gs_det_check(op, n, hwo, outer_div, inner):
    """The deterministic splat's limit: a texel of grad_input receives at most copies * Ho * Wo contributions."""
    copies = max(1, min(n, -(-outer_div // inner)))
    if copies * hwo > _SPLAT_MAX_CONTRIBUTIONS:
        raise _det_unserved(op, f"a texel of grad_input may receive {copies * hwo} > 2^32 contributions")


def _gs_det_workspace(gi, n, nin, c, hi, wi, ho, wo, device):
    if gi is None:  # (the grid's gradient alone: written per pixel, nothing to sum)
        return None, 0
    return _det_workspace("grid_sample", "waldo_grid_sample2d_bwd_det_workspace_bytes", (n, nin, c, hi, wi, ho, wo),
                          device)


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, grid, delta, outer_div, inner, want_mask=False):
        _lib.check_cuda(inp, grid)
        inp = _c(inp)
        grid = _c(grid)
        nin, c, hi, wi = inp.shape
        n, ho, wo, two = grid.shape
        assert two == 2
        if outer_div is None:
            if nin != n:
                raise _lib.WaldoHipError(f"grid_sample: batch mismatch {nin} vs {n}")
            outer_div = inner = max(n, 1)
        out = inp.new_empty(n, c, ho, wo)
        mask = inp.new_empty(n, 1, ho, wo) if want_mask else None
        if want_mask:
            _lib.launch("waldo_grid_sample2d_ex_fwd", inp.device, inp, grid, out, mask, n, c, hi, wi, ho, wo,
                        float(delta), outer_div, inner, max(n, 1), max(n, 1), max(n, 1), max(n, 1), 0, 1.0, 0.0)
        else:
            _lib.launch("waldo_grid_sample2d_fwd", inp.device, inp, grid, out, n, c, hi, wi, ho, wo, float(delta),
                        outer_div, inner, max(n, 1), max(n, 1))
        ctx.save_for_backward(inp, grid)
        ctx.cfg = (float(delta), outer_div, inner)
        ctx.det = is_deterministic()
        if ctx.det and ctx.needs_input_grad[0]:
            _gs_det_check("grid_sample", n, ho * wo, outer_div, inner)
        if want_mask:
            ctx.mark_non_differentiable(mask)
            return out, mask
        return out

    @staticmethod
    def backward(ctx, grad_out, _grad_mask=None):
        inp, grid = ctx.saved_tensors
        delta, outer_div, inner = ctx.cfg
        grad_out = _c(grad_out)
        nin, c, hi, wi = inp.shape
        n, ho, wo, _ = grid.shape
        # grad_input: overwritten by the deterministic kernel, accumulated into with atomics by the other
        gi = (torch.empty_like if ctx.det else torch.zeros_like)(inp) if ctx.needs_input_grad[0] else None
        gg = torch.empty_like(grid) if ctx.needs_input_grad[1] else None
        head, tail = (inp, grid, grad_out, gi, gg, n), (c, hi, wi, ho, wo, delta, outer_div, inner)
        if ctx.det:
            ws, nb = _gs_det_workspace(gi, n, nin, c, hi, wi, ho, wo, inp.device)
            _lib.launch("waldo_grid_sample2d_bwd_det", inp.device, *head, nin, *tail, ws, nb)
        else:
            _lib.launch("waldo_grid_sample2d_bwd", inp.device, *head, *tail)
        return gi, gg, None, None, None, None


def grid_sample(inp, grid, delta=0.0, broadcast=None, grid_repeat=None, return_mask=False, out=None):
    """``F.grid_sample(inp + delta, grid) - delta`` with the PyTorch defaults (bilinear, zeros,
    align_corners=False).  inp (Nin, C, Hi, Wi), grid (N, Ho, Wo, 2) -> (N, C, Ho, Wo).

    broadcast=(outer_div, inner): input map used by output n is
    ``(n // outer_div) * inner + n % inner`` -- the reference's ``.expand`` over time
    (models/nets/lvd.py:544,555) without materialising the copies.

    grid_repeat=(n_out, outer_div, inner): the same map for the GRID -- ``grid`` holds (Ng, Ho, Wo, 2) maps and
    output n of ``n_out`` reads map ``(n // outer_div) * inner + n % inner``: the predicted frames' grids
    repeated over the contexts (lvd.py:665-668) without the copies.  Inference only (no gradient).

    return_mask: also return ``grid_sample(ones_like(inp[:, :1]), grid)`` (N, 1, Ho, Wo) -- the warped all-ones image
    of ``Warper.grid_to_flow_ctx``'s ghost test (lvd.py:785-791), a by-product of the same taps (no gradient).

    out=(tensor, group, stride, offset): write output map n into slot ``(n // group) * stride + offset + n % group``
    of ``tensor`` (slots, C, Ho, Wo) instead of a tensor of its own -- the two calls of ``Warper.layer_to_output``
    (lvd.py:533-537) then fill the concatenated tensor directly.  Inference only; returns ``tensor``."""
    if grid_repeat is not None or out is not None:
        if torch.is_grad_enabled() and (inp.requires_grad or grid.requires_grad):
            raise _lib.WaldoHipError("grid_sample: grid_repeat / out are forward only (no gradient flows through them)")
        _lib.check_cuda(inp, grid)
        inp, grid = _c(inp.detach()), _c(grid.detach())
        nin, c, hi, wi = inp.shape
        ng, ho, wo, _ = grid.shape
        if grid_repeat is not None:
            n_out, god, gin = (int(v) for v in grid_repeat)
        else:
            n_out, god, gin = ng, max(ng, 1), max(ng, 1)
        od, inn = broadcast if broadcast is not None else (max(n_out, 1), max(n_out, 1))
        if god < 1 or gin < 1 or (n_out > 0 and ((n_out - 1) // god) * gin + min(gin, n_out) > ng) or \
                (broadcast is None and nin != n_out):
            raise _lib.WaldoHipError(f"grid_sample: grid_repeat {grid_repeat} against {ng} grids / {nin} inputs")
        if out is not None:
            dst, grp, stride, off = out[0], int(out[1]), int(out[2]), int(out[3])
            _lib.check_cuda(dst)
            slots = ((n_out - 1) // grp) * stride + off + min(grp, n_out) if n_out > 0 else 0
            if not dst.is_contiguous() or dst.dtype != inp.dtype or tuple(dst.shape[-3:]) != (c, ho, wo) or \
                    dst.numel() < slots * c * ho * wo or grp < 1 or off < 0 or off + grp > stride:
                raise _lib.WaldoHipError(f"grid_sample: out tensor {tuple(dst.shape)} does not hold slots "
                                         f"(group {grp}, stride {stride}, offset {off}) of {n_out} maps of {(c, ho, wo)}")
            res = dst
        else:
            grp, stride, off = max(n_out, 1), max(n_out, 1), 0
            res = inp.new_empty(n_out, c, ho, wo)
        mask = inp.new_empty(n_out, 1, ho, wo) if return_mask else None
        if return_mask or out is not None:
            _lib.launch("waldo_grid_sample2d_ex_fwd", inp.device, inp, grid, res, mask, n_out, c, hi, wi, ho, wo,
                        float(delta), od, inn, god, gin, grp, stride, off, 1.0, 0.0)
        else:
            _lib.launch("waldo_grid_sample2d_fwd", inp.device, inp, grid, res, n_out, c, hi, wi, ho, wo, float(delta),
                        od, inn, god, gin)
        return (res, mask) if return_mask else res
    od, inn = broadcast if broadcast is not None else (None, None)
    return _GridSample.apply(inp, grid, delta, od, inn, bool(return_mask))


class _LayersToOutput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj, bg, grid_obj, grid_bg, delta_obj, delta_bg, obj_bc, bg_bc, pre, want_mask):
        nf, h, w, _ = grid_bg.shape
        no = grid_obj.shape[0] // max(nf, 1)
        nl = no + 1
        c = obj.shape[1]
        out = obj.new_empty(nf, nl, c, h, w)
        mask = obj.new_empty(nf * no, 1, h, w) if want_mask else None
        calls = ((obj, grid_obj, mask, nf * no, delta_obj, obj_bc, (no, nl, 1)),
                 (bg, grid_bg, None, nf, delta_bg, bg_bc, (1, nl, 0)))
        for inp, grid, msk, n, delta, bc, slots in calls:
            if n == 0:  # (no frames, or no objects: the background alone)
                continue
            od, inn = bc if bc is not None else (max(n, 1), max(n, 1))
            _lib.launch("waldo_grid_sample2d_ex_fwd", obj.device, inp, grid, out, msk, n, c, inp.shape[2], inp.shape[3],
                        h, w, float(delta), od, inn, max(n, 1), max(n, 1), *slots, float(pre[0]), float(pre[1]))
        ctx.save_for_backward(obj, bg, grid_obj, grid_bg)
        ctx.cfg = (float(delta_obj), float(delta_bg), obj_bc, bg_bc, (float(pre[0]), float(pre[1])), no)
        ctx.det = is_deterministic()
        if ctx.det:
            for need, n, bc in ((ctx.needs_input_grad[0], nf * no, obj_bc), (ctx.needs_input_grad[1], nf, bg_bc)):
                if need and n > 0:
                    _gs_det_check("layers_to_output", n, h * w, *(bc if bc is not None else (n, n)))
        if want_mask:
            ctx.mark_non_differentiable(mask)
            return out, mask
        return out

    @staticmethod
    def backward(ctx, grad_out, _grad_mask=None):
        obj, bg, grid_obj, grid_bg = ctx.saved_tensors
        delta_obj, delta_bg, obj_bc, bg_bc, pre, no = ctx.cfg
        nf, h, w, _ = grid_bg.shape
        nl = no + 1
        c = obj.shape[1]
        grad_out = _c(grad_out)
        need = ctx.needs_input_grad
        res = []
        # (overwritten by the deterministic kernels, accumulated into by the others)
        gis = (_empty_like_each if ctx.det else _zeros_like_each)(obj if need[0] else None, bg if need[1] else None)
        calls = ((obj, grid_obj, nf * no, delta_obj, obj_bc, (no, nl, 1), gis[0], need[2]),
                 (bg, grid_bg, nf, delta_bg, bg_bc, (1, nl, 0), gis[1], need[3]))
        for inp, grid, n, delta, bc, slots, gi, want_g in calls:
            gg = torch.empty_like(grid) if want_g else None
            if (ctx.det or n > 0) and (gi is not None or want_g):
                nin, _, hi, wi = inp.shape
                od, inn = bc if bc is not None else (max(n, 1), max(n, 1))
                head, tail = (inp, grid, grad_out, gi, gg, n), (c, hi, wi, h, w, delta, od, inn, *slots, pre[0], pre[1])
                if ctx.det:
                    ws, nb = _gs_det_workspace(gi, n, nin, c, hi, wi, h, w, obj.device)
                    _lib.launch("waldo_grid_sample2d_ex_bwd_det", obj.device, *head, nin, *tail, ws, nb)
                else:
                    _lib.launch("waldo_grid_sample2d_ex_bwd", obj.device, *head, *tail)
            res.append((gi, gg))
        return res[0][0], res[1][0], res[0][1], res[1][1], None, None, None, None, None, None


def layers_to_output(obj, bg, grid_obj, grid_bg, delta_obj=0.0, delta_bg=0.0, obj_broadcast=None, bg_broadcast=None,
                     pre=(1.0, 0.0), return_mask=False):
    """``Warper.layer_to_output`` (models/nets/lvd.py:533-559) as ONE differentiable op: the objects' maps and the
    background's warped straight into the tensor the reference concatenates,

        torch.cat([grid_sample(bg', grid_bg, delta_bg)[:, None], grid_sample(obj', grid_obj, delta_obj).view(F, No, ...)], 1)

    obj (Nin_o, C, Ho, Wo) with grid_obj (F * No, H, W, 2), bg (Nin_b, C, Hb, Wb) with grid_bg (F, H, W, 2) ->
    (F, No + 1, C, H, W), the background at layer 0.  ``*_broadcast`` = (outer_div, inner) as in ``grid_sample`` (the
    reference's ``.expand`` over time).  ``pre`` = (scale, bias): the images warped are ``scale * obj + bias`` and
    ``scale * bg + bias`` -- ``grid_to_flow`` warps ``(alpha + 1) / 2`` (lvd.py:602-606, 716-720) -- without being written
    first; the gradients returned are those of ``obj`` / ``bg``.  ``return_mask``: also the warped all-ones canvas of
    the objects' grids (F * No, 1, H, W) (``grid_sample(..., return_mask=True)``; no gradient).

    Forward: two launches that write disjoint slots of one tensor (no ``cat``); backward: two launches that read their
    slots of the tensor's gradient (no copies of its two slices)."""
    _lib.check_cuda(obj, bg, grid_obj, grid_bg)
    obj, bg, grid_obj, grid_bg = _c(obj), _c(bg), _c(grid_obj), _c(grid_bg)
    nf, h, w, two = grid_bg.shape
    ngo = grid_obj.shape[0]
    if two != 2 or grid_obj.dim() != 4 or tuple(grid_obj.shape[1:]) != (h, w, 2) or obj.dim() != 4 or bg.dim() != 4 or \
            obj.shape[1] != bg.shape[1] or (nf == 0 and ngo != 0) or (nf > 0 and ngo % nf != 0) or obj.dtype != bg.dtype:
        raise _lib.WaldoHipError(f"layers_to_output: obj {tuple(obj.shape)} / grid_obj {tuple(grid_obj.shape)} against "
                                 f"bg {tuple(bg.shape)} / grid_bg {tuple(grid_bg.shape)}")
    for name, inp, n, bc in (("obj", obj, ngo, obj_broadcast), ("bg", bg, nf, bg_broadcast)):
        if bc is None:
            if inp.shape[0] != n:
                raise _lib.WaldoHipError(f"layers_to_output: {inp.shape[0]} {name} images for {n} grids")
        else:
            od, inn = int(bc[0]), int(bc[1])
            if od < 1 or inn < 1 or (n > 0 and ((n - 1) // od) * inn + min(inn, n) > inp.shape[0]):
                raise _lib.WaldoHipError(f"layers_to_output: {name} broadcast {bc} of {n} maps over {inp.shape[0]} images")
    obj_bc = None if obj_broadcast is None else (int(obj_broadcast[0]), int(obj_broadcast[1]))
    bg_bc = None if bg_broadcast is None else (int(bg_broadcast[0]), int(bg_broadcast[1]))
    return _LayersToOutput.apply(obj, bg, grid_obj, grid_bg, float(delta_obj), float(delta_bg), obj_bc, bg_bc,
                                 (float(pre[0]), float(pre[1])), bool(return_mask))


# --------------------------------------------------------------------------------------
# A6: occlusion product
# --------------------------------------------------------------------------------------
class _OccComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, occ, occ_div):
        _lib.check_cuda(alpha, occ)
        alpha = _c(alpha)
        occ = _c(occ)
        m, nl, hw = alpha.shape
        out = torch.empty_like(alpha)
        _lib.launch("waldo_occ_composite_fwd", alpha.device, alpha, occ, out, m, nl, hw, occ_div)
        ctx.save_for_backward(alpha, occ)
        ctx.occ_div = occ_div
        ctx.det = is_deterministic()
        return out

    @staticmethod
    def backward(ctx, grad_out):
        alpha, occ = ctx.saved_tensors
        grad_out = _c(grad_out)
        m, nl, hw = alpha.shape
        ga = torch.empty_like(alpha)
        det = ctx.det and ctx.needs_input_grad[1]  # (grad_alpha is written per pixel: only grad_occ is a sum)
        go = (torch.empty_like if det else torch.zeros_like)(occ) if ctx.needs_input_grad[1] else None
        args = (alpha, occ, grad_out, ga, go, m, nl, hw, ctx.occ_div)
        if det:
            ws, nb = _det_workspace("occ_composite", "waldo_occ_composite_bwd_det_workspace_bytes", (m, nl, hw),
                                    alpha.device)
            if occ.shape[0] * ctx.occ_div != m:  # (matrices no map reads: the kernel overwrites those it sums)
                go.zero_()
            _lib.launch("waldo_occ_composite_bwd_det", alpha.device, *args, ws, nb)
        else:
            _lib.launch("waldo_occ_composite_bwd", alpha.device, *args)
        return ga, go, None


def occ_composite(alpha, occ, occ_div=1):
    """out[m, j] = alpha[m, j] * prod_i (1 - alpha[m, i] * occ[m // occ_div, i, j]).
    alpha (M, L, h, w) or (M, L, HW) in [0, 1]; occ (M // occ_div, L, L).
    The (1 - alpha * occ).prod(dim) * alpha pattern of models/nets/lvd.py:651-652,764-765,809."""
    shape = alpha.shape
    a3 = alpha.reshape(shape[0], shape[1], -1)
    return _OccComposite.apply(a3, occ, int(occ_div)).view(shape)


# --------------------------------------------------------------------------------------
# f2: producers of the path's inputs (csrc/producers.hip)
# --------------------------------------------------------------------------------------
class _ComputeOcc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, eps):
        _lib.check_cuda(score)
        score = _c(score)
        m, no = score.shape
        occ = score.new_empty(m, no + 1, no + 1)
        _lib.launch("waldo_compute_occ_fwd", score.device, score, occ, m, no, float(eps))
        ctx.save_for_backward(score)
        ctx.eps = float(eps)
        return occ

    @staticmethod
    def backward(ctx, grad_occ):
        (score,) = ctx.saved_tensors
        grad_occ = _c(grad_occ)
        m, no = score.shape
        gs = torch.empty_like(score)
        _lib.launch("waldo_compute_occ_bwd", score.device, score, grad_occ, gs, m, no, ctx.eps)
        return gs, None


def compute_occ(occ_score, eps=1e-6):
    """LVD.compute_occ (models/nets/lvd.py:59-68): occ_score (..., No) -> (..., No+1, No+1)."""
    lead = occ_score.shape[:-1]
    no = occ_score.shape[-1]
    occ = _ComputeOcc.apply(occ_score.reshape(-1, no).float(), eps)
    return occ.view(*lead, no + 1, no + 1)


class _AlphaHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, prior, mask, scale, bias, has_alpha, mode):
        _lib.check_cuda(x, prior, mask)
        x = _c(x)
        prior = _c(prior) if prior is not None else None
        mask = _c(mask) if mask is not None else None
        n, c, h, w = x.shape
        if prior is not None and prior.numel() != h * w:
            raise _lib.WaldoHipError(f"alpha_head: prior has {prior.numel()} elements, expected {h}x{w}")
        if mask is not None and mask.numel() != h * w * scale * scale:
            raise _lib.WaldoHipError(f"alpha_head: mask has {mask.numel()} elements, expected "
                                     f"{h * scale}x{w * scale}")
        out = x.new_empty(n, c, h * scale, w * scale)
        _lib.launch("waldo_alpha_head_fwd", x.device, x, prior, mask, out, n, c, h, w, scale, float(bias),
                    int(has_alpha), mode)
        ctx.save_for_backward(x, prior, mask)
        ctx.cfg = (scale, float(bias), int(has_alpha), mode)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, prior, mask = ctx.saved_tensors
        scale, bias, has_alpha, mode = ctx.cfg
        grad_out = _c(grad_out)
        n, c, h, w = x.shape
        gx = torch.empty_like(x)
        _lib.launch("waldo_alpha_head_bwd", x.device, x, prior, mask, grad_out, gx, n, c, h, w, scale, bias, has_alpha,
                    mode)
        return gx, None, None, None, None, None, None


def disocc_test(layer_max):
    """Synthesizer.predict's disocclusion test (models/synthesizer.py:447-450): ``layer_max`` (B, Tc, Tp, H, W) =
    ``alpha_ctx.max(dim=3)[0]`` -> ``dmax`` (B, Tp, H, W) with ``dmax[dmax - dmin > 1] = 0``, max / min over the
    contexts (NaN-propagating as torch's).  One pass; inference only."""
    _lib.check_cuda(layer_max)
    if layer_max.ndim != 5:
        raise _lib.WaldoHipError(f"disocc_test: layer_max {tuple(layer_max.shape)} is not (B, Tc, Tp, H, W)")
    layer_max = _c(layer_max.detach())
    b, tc, tp, h, w = layer_max.shape
    out = layer_max.new_empty(b, tp, h, w)
    _lib.launch("waldo_disocc_test_fwd", layer_max.device, layer_max, out, b, tc, tp, h * w)
    return out


def alpha_head(img, prior=None, mask=None, scale=1, bias=0.0, has_alpha=True, remove=False, freeze=False):
    """ImageDecoder.forward's tail (models/nets/lvd.py:245-254: ``+ init_bias``, ``tanh`` and the
    ``circle`` prior on the last channel, ``scale(img, scale_factor)``) fused with the alpha
    arithmetic of ``LVD.forward(mode="estimate_alpha_grid_occ")`` (lvd.py:128-132: ``remove_obj`` /
    ``freeze_obj`` / ``obj_alpha_mask``).  img (N, C, h, w) -> (N, C, h*scale, w*scale)."""
    mode = 2 if freeze else (1 if remove else 0)
    return _AlphaHead.apply(img.float(), prior, mask, int(scale), bias, bool(has_alpha), mode)


class _PoseAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, mul6, bias6, base, mul_delta, pts_mul):
        _lib.check_cuda(pose, mul6, bias6, base)
        pose, mul6, bias6, base = _c(pose), _c(mul6), _c(bias6), _c(base)
        r, d = pose.shape
        p = (d - 6) // 2
        if d != 6 + 2 * p or base.numel() != 2 * p or mul6.numel() != 6 or bias6.numel() != 6:
            raise _lib.WaldoHipError(f"pose_affine: inconsistent shapes pose={tuple(pose.shape)} "
                                     f"base={tuple(base.shape)}")
        out = pose.new_empty(r, p, 2)
        _lib.launch("waldo_pose_affine_fwd", pose.device, pose, mul6, bias6, base, out, r, p, float(mul_delta),
                    float(pts_mul))
        ctx.save_for_backward(pose, mul6, bias6, base)
        ctx.cfg = (float(mul_delta), float(pts_mul))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        pose, mul6, bias6, base = ctx.saved_tensors
        grad_out = _c(grad_out)
        r, d = pose.shape
        gp = torch.empty_like(pose)
        _lib.launch("waldo_pose_affine_bwd", pose.device, pose, mul6, bias6, base, grad_out, gp, r, (d - 6) // 2,
                    ctx.cfg[0], ctx.cfg[1])
        return gp, None, None, None, None, None


def pose_affine(pose, mul6, bias6, base_pts, mul_delta=1.0, pts_mul=1.0):
    """The pose heads' affine (models/nets/flp.py:259-273): pose (..., 6 + 2P) -> control points
    (..., P, 2) = [pts_mul * base_pts + mul_delta * pose[6:], 1] @ (mul6 * pose[:6] + bias6)."""
    lead = pose.shape[:-1]
    d = pose.shape[-1]
    out = _PoseAffine.apply(pose.reshape(-1, d).float(), mul6.reshape(-1).float(), bias6.reshape(-1).float(),
                            base_pts.reshape(-1, 2).float(), mul_delta, pts_mul)
    return out.view(*lead, (d - 6) // 2, 2)


# --------------------------------------------------------------------------------------
# A12: WIF fusion epilogue
# --------------------------------------------------------------------------------------
# element types of the *_dt entry points (include/waldo_hip.h: enum waldo_dtype)
_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _dt_entry(name, *dtypes):
    """(entry point, its trailing arguments) for buffers of ``dtypes``: ``name`` and nothing when every one is fp32,
    else ``name + "_dt"`` and the dtype codes.  fp32 work keeps launching the fp32 entry point under its own name
    (KernelTimer keys on it)."""
    codes = tuple(_DTYPE_CODE[d] for d in dtypes)
    return (name + "_dt", codes) if any(codes) else (name, ())


class _WifFuse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vid, net, ab):
        _lib.check_cuda(vid, net, half=True)  # (fp16 / bf16 too: a UNet under autocast)
        vid, net = _c(vid), _c(net)
        b, t, tc, c, h, w = vid.shape
        co = net.shape[3]
        if tuple(net.shape) != (b, t, tc, co, h, w):
            raise _lib.WaldoHipError(f"wif_fuse: shapes {tuple(vid.shape)} vs {tuple(net.shape)}")
        out = vid.new_empty(b, t, 3, h, w, dtype=torch.float32)
        name, codes = _dt_entry("waldo_wif_fuse_fwd", vid.dtype, net.dtype)
        _lib.launch(name, vid.device, vid, net, out, b * t, tc, c, co, h * w, int(bool(ab)), *codes)
        ctx.save_for_backward(vid, net, out)
        ctx.ab = int(bool(ab))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        vid, net, out = ctx.saved_tensors
        b, t, tc, c, h, w = vid.shape
        co = net.shape[3]
        grad_out = _c(grad_out)
        gv = torch.empty_like(vid) if ctx.needs_input_grad[0] else None
        gn = torch.empty_like(net) if ctx.needs_input_grad[1] else None
        name, codes = _dt_entry("waldo_wif_fuse_bwd", vid.dtype, net.dtype)
        _lib.launch(name, vid.device, vid, net, out, grad_out, gv, gn, b * t, tc, c, co, h * w, ctx.ab, *codes)
        return gv, gn, None


def wif_fuse(vid, net_out, ab=True):
    """Fusion epilogue of WIF.forward with ii_score (models/nets/wif.py:49-54).
    vid (B, T, Tc, C, H, W): the UNet input after the permute; net_out (B, T, Tc, 4|5, H, W).  Each of them fp32, fp16
    or bf16 (a 16-bit raw_output, a UNet under autocast): widened to fp32 on load, the arithmetic is the fp32 one.
    The result is fp32; the gradients come back in their inputs' types (the fp32 gradients rounded to nearest-even)."""
    return _WifFuse.apply(vid, net_out, ab)


# --------------------------------------------------------------------------------------
# A9: the two HD passes of Warper.grid_to_flow_ctx / grid_to_flow (forward only)
# --------------------------------------------------------------------------------------
class _LytDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, lyt, cls, min_cls, first_obj):
        b, tw, la, h, w = alpha.shape
        nl = lyt.shape[2]
        no = la - first_obj
        dev = alpha.device
        dist = alpha.new_empty(b, no, nl)
        mean = alpha.new_empty(b, no, nl)
        total = alpha.new_empty(b, no)
        wsb = _lib.query("waldo_lyt_dist_workspace_bytes", b, tw, no, nl, h, w)
        ws = alpha.new_empty(max(wsb, 4) // 4)
        _lib.launch("waldo_lyt_dist_fwd", dev, alpha, lyt, lyt.stride(0), lyt.stride(1), cls, float(min_cls), dist, mean,
                    total, ws, b, tw, la, first_obj, no, nl, h, w)
        ctx.save_for_backward(alpha, lyt, cls, dist, mean, total)
        ctx.cfg = (float(min_cls), first_obj)
        ctx.mark_non_differentiable(mean, total)
        return dist, mean, total

    @staticmethod
    def backward(ctx, g_dist, _g_mean, _g_total):
        alpha, lyt, cls, dist, mean, total = ctx.saved_tensors
        min_cls, first_obj = ctx.cfg
        b, tw, la, h, w = alpha.shape
        nl = lyt.shape[2]
        no = la - first_obj
        dev = alpha.device
        g_dist = _c(g_dist)
        g_alpha = torch.empty_like(alpha)
        g_cls = torch.empty_like(cls) if cls is not None else None
        wsb = _lib.query("waldo_lyt_dist_workspace_bytes", b, tw, no, nl, h, w)
        ws = alpha.new_empty(max(wsb, 4) // 4)
        _lib.launch("waldo_lyt_dist_bwd", dev, g_dist, alpha, lyt, lyt.stride(0), lyt.stride(1), cls, min_cls, dist, mean,
                    total, g_alpha, g_cls, ws, b, tw, la, first_obj, no, nl, h, w)
        return g_alpha, None, g_cls, None, None


def lyt_dist(alpha, lyt, cls=None, min_cls=0.0, first_obj=1):
    """Class distribution of every object for the layout filter (models/nets/lvd.py:624-634 /
    731-746).  alpha (B, Tw, L, H, W) projected alpha in [0, 1], objects = layers first_obj .. L-1;
    lyt (B, Tw, Nl, H, W) layout logits at the same raster (any batch / frame strides: a channel
    slice of the input works without a copy); cls (B, No, Nl) = the reference's ``cls`` when
    ``weight_cls`` is set, else None.  Returns dist (B, No, Nl).  Differentiable w.r.t. alpha and
    cls; the layout is data."""
    _lib.check_cuda(alpha, lyt, cls)
    alpha = _c(alpha)
    lyt = lyt.detach()
    b, tw, la, h, w = alpha.shape
    if lyt.dim() != 5 or tuple(lyt.shape[:2]) != (b, tw) or tuple(lyt.shape[3:]) != (h, w):
        raise _lib.WaldoHipError(f"lyt_dist: lyt {tuple(lyt.shape)} does not match alpha {tuple(alpha.shape)}")
    if lyt.stride(4) != 1 or lyt.stride(3) != w or lyt.stride(2) != h * w:
        lyt = lyt.contiguous()
    if cls is not None:
        cls = _c(cls)
        if tuple(cls.shape) != (b, la - first_obj, lyt.shape[2]):
            raise _lib.WaldoHipError(f"lyt_dist: cls {tuple(cls.shape)} is not (B, No, Nl)")
    return _LytDist.apply(alpha, lyt, cls, float(min_cls), int(first_obj))[0]


def _flow_ctx_alpha_fwd(alpha_lr, input, dist, occ, tw, chan_off, scale, want_alpha=True, want_bits=False):
    """The forward launch of ``flow_ctx_alpha`` on checked, contiguous arguments (``input``: the fp32 clip or a
    ``PackedClip``) -> (a01, alpha or None, layer_bits or None)."""
    n, nl, h, w = alpha_lr.shape
    b, t, c, hd, wd = input.shape
    dev = alpha_lr.device
    a01 = alpha_lr.new_empty(n, nl, hd, wd)
    alpha = alpha_lr.new_empty(n, nl, hd, wd) if want_alpha else None
    bits = torch.empty(n, hd, (wd + 63) // 64, dtype=torch.int32, device=dev) if want_bits else None
    if isinstance(input, PackedClip):
        _lib.launch("waldo_flow_ctx_alpha_packed_fwd", dev, alpha_lr, _packed_data(input, "flow_ctx_alpha"), dist, occ,
                    a01, alpha, bits, b, t, tw, nl, input.num_lyt, h, w, scale)
    else:
        _lib.launch("waldo_flow_ctx_alpha_fwd", dev, alpha_lr, input, dist, occ, a01, alpha, bits, b, t, tw, nl,
                    dist.shape[2] if dist is not None else 0, c, chan_off, h, w, scale)
    return a01, alpha, bits


class _FlowCtxAlpha(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha_lr, input, dist, occ, tw, chan_off, scale):
        a01, out, _ = _flow_ctx_alpha_fwd(alpha_lr, input, dist, occ, tw, chan_off, scale)
        ctx.save_for_backward(alpha_lr, input, dist, occ)
        ctx.cfg = (tw, chan_off, scale)
        ctx.det = is_deterministic()
        ctx.set_materialize_grads(False)  # backward below handles a missing gradient of either output
        return a01, out

    @staticmethod
    def backward(ctx, g_a01, g_out):
        alpha_lr, input, dist, occ = ctx.saved_tensors
        tw, chan_off, scale = ctx.cfg
        n, nl, h, w = alpha_lr.shape
        b, t, c, hd, wd = input.shape
        ncls = dist.shape[2] if dist is not None else 0
        # alpha_out = 2 a01 - 1
        if g_a01 is None and g_out is None:
            return None, None, None, None, None, None, None
        # (the kernel reads g_a01 + 2 g_out itself: no pass over (B*Tw, L, Hd, Wd) to add them first)
        g_a01 = _c(g_a01) if g_a01 is not None else None
        g_out = _c(g_out) if g_out is not None else None
        g_lr = torch.empty_like(alpha_lr)
        summed = (dist if (dist is not None and ctx.needs_input_grad[2]) else None, occ if ctx.needs_input_grad[3] else None)
        if ctx.det:  # (the sums are overwritten; the workspace travels with its size)
            name = "waldo_flow_ctx_alpha_bwd_det"
            g_dist, g_occ = _empty_like_each(*summed)
            ws = _det_workspace("flow_ctx_alpha", "waldo_flow_ctx_alpha_bwd_det_workspace_bytes",
                                (b, tw, nl, ncls, h, w, scale), alpha_lr.device)
        else:
            name = "waldo_flow_ctx_alpha_bwd"
            g_dist, g_occ = _zeros_like_each(*summed)
            ws = (alpha_lr.new_empty(n, nl, hd, wd) if scale > 1 else None,)
        _lib.launch(name, alpha_lr.device, alpha_lr, input, dist, occ, g_a01, g_out, g_lr, g_dist, g_occ, *ws, b, t, tw,
                    nl, ncls, c, chan_off, h, w, scale)
        return g_lr, None, g_dist, g_occ, None, None, None


def flow_ctx_alpha(alpha_lr, input, dist, occ, tw, chan_off, scale, want_alpha=True, want_bits=False):
    """Upsampling + layout filter + first occlusion product (models/nets/lvd.py:731-766).
    alpha_lr (B*Tw, L, H, W) in [0, 1]; input (B, T, C, Hd, Wd) with the layout logits in channels
    [chan_off, chan_off + Nl); dist (B, L-1, Nl) or None (no filter); occ (B, T, L, L).
    Returns (a01, alpha) of shape (B*Tw, L, Hd, Wd): the composited alpha in [0, 1] and 2a - 1.
    Differentiable w.r.t. alpha_lr, dist and occ (the frames / layouts in ``input`` are data).
    ``want_alpha=False`` (no autograd): ``alpha`` is not written and comes back as None -- ``Synthesizer.predict``'s
    reconstruction drops it (synthesizer.py:445), and it is as large as ``a01``.
    ``want_bits`` (no autograd): a third result, ``layer_bits`` (B*Tw, Hd, ceil(Wd / 64)) int32 -- bit l of a word: layer
    l of ``a01`` is non-zero somewhere in that 64-pixel row segment -- for ``flow_ctx_warp(..., layer_bits=...)`` on the
    path without a ghost mask (``Warper.grid_to_flow``).
    ``input`` may be a ``PackedClip`` (``chan_off`` 3), without autograd: the layout logits are read from its class
    bytes (``waldo_flow_ctx_alpha_packed_fwd``), with the bits of the call on its unpacked form."""
    packed = isinstance(input, PackedClip)
    _lib.check_cuda(alpha_lr, occ, *(() if packed else (input,)))
    alpha_lr, input, occ = _c(alpha_lr), (input if packed else _c(input.detach())), _c(occ)
    n, nl, h, w = alpha_lr.shape
    b, t, c, hd, wd = input.shape
    if n != b * tw or tuple(occ.shape) != (b, t, nl, nl) or hd != h * scale or wd != w * scale:
        raise _lib.WaldoHipError(
            f"flow_ctx_alpha: inconsistent shapes alpha_lr={tuple(alpha_lr.shape)} input={tuple(input.shape)} "
            f"occ={tuple(occ.shape)} tw={tw} scale={scale}")
    if dist is not None:
        dist = _c(dist)
        if tuple(dist.shape[:2]) != (b, nl - 1):
            raise _lib.WaldoHipError(f"flow_ctx_alpha: dist {tuple(dist.shape)} is not (B, L-1, Nl)")
    no_grad = not (torch.is_grad_enabled() and (alpha_lr.requires_grad or occ.requires_grad or
                                                (dist is not None and dist.requires_grad)))
    if packed:
        if not no_grad:
            raise _lib.WaldoHipError("flow_ctx_alpha: no gradient flows through a packed clip's pass; unpack() it")
        if dist is not None and int(chan_off) != 3:
            raise _lib.WaldoHipError(f"flow_ctx_alpha: a packed clip's layout channels start at 3, not {chan_off}")
    if packed or (no_grad and (not want_alpha or want_bits)):
        a01, alpha, bits = _flow_ctx_alpha_fwd(alpha_lr, input, dist, occ, tw, chan_off, scale, want_alpha, want_bits)
        return (a01, alpha, bits) if want_bits else (a01, alpha)
    res = _FlowCtxAlpha.apply(alpha_lr, input, dist, occ, tw, chan_off, scale)
    return (*res, None) if want_bits else res


def _flow_ctx_warp_fwd(name, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale, layer_max, status_ptr, bits_ptr,
                       alpha_out, *raw_args):
    """The forward launch of ``flow_ctx_warp`` (``alpha_out``: alpha_ctx) and of ``flow_ctx_warp_into_raw`` (``alpha_out``:
    raw and score; ``raw_args``: the raw-slot arguments that follow the shape) on checked, contiguous arguments ->
    (flow, disocc, amax or None)."""
    m, nl, _, h, w = flow_lr.shape
    b, tc, tp = ctx_ts.shape
    t = occ.shape[1]
    hd, wd = a01.shape[-2:]
    flow = flow_lr.new_empty(m, 2, hd, wd)
    disocc = flow_lr.new_empty(m, hd, wd)
    amax = flow_lr.new_empty(m, hd, wd) if layer_max else None
    _lib.launch(name, flow_lr.device, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, flow, *alpha_out, disocc, amax,
                bits_ptr, status_ptr, b, t, tw, tc, tp, nl, h, w, scale, *raw_args)
    return flow, disocc, amax


class _FlowCtxWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale, layer_max, status_ptr, bits_ptr=None):
        m, nl = flow_lr.shape[:2]
        tc, tp = ctx_ts.shape[1:]
        hd, wd = a01.shape[-2:]
        alpha_ctx = flow_lr.new_empty(m, nl, hd, wd)
        flow, disocc, amax = _flow_ctx_warp_fwd("waldo_flow_ctx_warp_fwd", flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw,
                                                scale, layer_max, status_ptr, bits_ptr, (alpha_ctx,))
        if amax is None:
            amax = flow_lr.new_empty(0)
        ctx.save_for_backward(flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ)
        ctx.cfg = (tw, scale)
        ctx.det = is_deterministic()
        if ctx.det and ctx.needs_input_grad[2] and tc * tp * hd * wd > _SPLAT_MAX_CONTRIBUTIONS:
            raise _det_unserved("flow_ctx_warp", f"a texel of grad_a01 may receive {tc * tp * hd * wd} > 2^32 contributions")
        ctx.mark_non_differentiable(amax)
        ctx.set_materialize_grads(False)  # unused outputs: None, not zero-filled tensors (the kernel takes NULL)
        return flow, alpha_ctx, disocc, amax

    @staticmethod
    def backward(ctx, g_flow, g_actx, g_dis, _g_amax):
        flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ = ctx.saved_tensors
        tw, scale = ctx.cfg
        m, nl, _, h, w = flow_lr.shape
        b, tc, tp = ctx_ts.shape
        t = occ.shape[1]
        hd, wd = a01.shape[-2:]
        g_flow = _c(g_flow) if g_flow is not None else None
        g_actx = _c(g_actx) if g_actx is not None else None
        g_dis = _c(g_dis) if g_dis is not None else None
        g_lr = torch.empty_like(flow_lr)
        summed = (a01 if ctx.needs_input_grad[2] else None, occ if ctx.needs_input_grad[5] else None)
        if ctx.det:  # (the sums are overwritten; the workspace travels with its size)
            name = "waldo_flow_ctx_warp_bwd_det"
            g_a01, g_occ = _empty_like_each(*summed)
            ws = _det_workspace("flow_ctx_warp", "waldo_flow_ctx_warp_bwd_det_workspace_bytes",
                                (b, tw, tc, tp, nl, h, w, scale), flow_lr.device)
        else:
            name = "waldo_flow_ctx_warp_bwd"
            g_a01, g_occ = _zeros_like_each(*summed)
            ws = (flow_lr.new_empty(m, nl, 2, hd, wd) if scale > 1 else None,)
        _lib.launch(name, flow_lr.device, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, g_flow, g_actx, g_dis, g_lr, g_a01,
                    g_occ, *ws, b, t, tw, tc, tp, nl, h, w, scale)
        return g_lr, None, g_a01, None, None, g_occ, None, None, None, None, None


def _flow_ctx_warp_args(fn, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale):
    _lib.check_cuda(flow_lr, a01, occ)
    if not (ctx_ts.is_cuda and pred_ts.is_cuda):
        raise _lib.WaldoHipError(f"{fn}: ctx_ts / pred_ts must be on the GPU")
    flow_lr, a01, occ = _c(flow_lr), _c(a01), _c(occ)
    ctx_ts, pred_ts = _c(ctx_ts.long()), _c(pred_ts.long())
    m, nl, _, h, w = flow_lr.shape
    b, tc, tp = ctx_ts.shape
    t = occ.shape[1]
    if m != b * tc * tp or pred_ts.numel() != tp or tuple(a01.shape) != (b * tw, nl, h * scale, w * scale) \
            or tuple(occ.shape) != (b, t, nl, nl):
        raise _lib.WaldoHipError(
            f"{fn}: inconsistent shapes flow_lr={tuple(flow_lr.shape)} a01={tuple(a01.shape)} "
            f"ctx_ts={tuple(ctx_ts.shape)} pred_ts={tuple(pred_ts.shape)} occ={tuple(occ.shape)}")
    if isobj_lr is not None:
        _lib.check_cuda(isobj_lr)
        isobj_lr = _c(isobj_lr.detach())
        if tuple(isobj_lr.shape) != (m, nl - 1, h, w):
            raise _lib.WaldoHipError(f"{fn}: isobj_lr {tuple(isobj_lr.shape)} is not (M, L-1, H, W)")
    return flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ


def _layer_bits_ptr(fn, layer_bits, a01):
    """``flow_ctx_alpha(..., want_bits=True)``'s map for this very ``a01`` (shape-checked), or NULL."""
    if layer_bits is None:
        return None
    n, _, hd, wd = a01.shape
    if not layer_bits.is_cuda or layer_bits.dtype != torch.int32 or not layer_bits.is_contiguous() or \
            tuple(layer_bits.shape) != (n, hd, (wd + 63) // 64):
        raise _lib.WaldoHipError(f"{fn}: layer_bits {tuple(layer_bits.shape)} {layer_bits.dtype} is not the int32 "
                                 f"(B*Tw, Hd, ceil(Wd / 64)) map of a01 {tuple(a01.shape)}")
    return layer_bits.data_ptr()


def flow_ctx_warp(flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale, layer_max=False, status=None,
                  layer_bits=None):
    """Context-alpha warp + ghost mask + disocclusion + second occlusion product + flow compositing
    (models/nets/lvd.py:784-818).  flow_lr (B*Tc*Tp, L, 2, H, W); isobj_lr (B*Tc*Tp, L-1, H, W) or None;
    a01 (B*Tw, L, Hd, Wd) from flow_ctx_alpha; ctx_ts (B, Tc, Tp) long; pred_ts (Tp) long;
    occ (B, T, L, L).  Returns flow (M, 2, Hd, Wd), alpha_ctx (M, L, Hd, Wd) in [-1, 1],
    disocc (M, Hd, Wd).  Differentiable w.r.t. flow_lr, a01 and occ (the thresholded ghost mask
    carries no gradient, as in the reference).  ``layer_max``: a fourth result, ``alpha_ctx.amax(dim=1)``
    (M, Hd, Wd) -- what Synthesizer.predict's disocclusion test computes from alpha_ctx (synthesizer.py:447) --
    as a by-product (no gradient).  ``ctx_ts`` must lie in [0, tw), ``pred_ts`` in [0, T): validated on the device
    (``status``: the caller's ``_lib.IndexStatus``, checked when the caller chooses; None: checked before returning).
    ``layer_bits``: ``flow_ctx_alpha(..., want_bits=True)``'s map for this ``a01`` -- without a ghost mask it lets the
    pass skip, per tile, the layers that are absent wherever the tile samples; the values do not depend on it."""
    flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ = _flow_ctx_warp_args("flow_ctx_warp", flow_lr, isobj_lr, a01, ctx_ts,
                                                                       pred_ts, occ, tw, scale)
    st, strict = _status(status)
    flow, alpha_ctx, disocc, amax = _FlowCtxWarp.apply(flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale,
                                                       bool(layer_max), st.ptr,
                                                       _layer_bits_ptr("flow_ctx_warp", layer_bits, a01))
    if strict:
        st.check(sync=True)
    return (flow, alpha_ctx, disocc, amax) if layer_max else (flow, alpha_ctx, disocc)


class RawSlots:
    """What ``flow_ctx_warp_into_raw`` leaves for ``frame_warp_fuse_raw``: the ``raw`` tensor of
    Warper.input_to_output, (B, Tp, Tc', C + L, Hd, Wd), with the alpha slots of its Tc contexts filled, and
    ``score`` (B, Tc, Tp, Hd, Wd) = the per-context sums of (alpha + 1) / 2 (lvd.py:841).  ``raw`` is fp32, bf16 or
    fp16 (``raw.dtype``); ``score`` is fp32 in every case."""

    def __init__(self, raw, score, channels, include_self):
        self.raw, self.score, self.channels, self.include_self = raw, score, channels, include_self


def flow_ctx_warp_into_raw(flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale, channels, include_self,
                           layer_max=False, status=None, layer_bits=None, raw_dtype=torch.float32):
    """``flow_ctx_warp`` for the caller that runs ``frame_warp_fuse_raw`` on the result next
    (LVD.forward(mode="decode_output"), lvd.py:141-153), WITHOUT autograd: ``alpha_ctx`` is written straight
    into the alpha slots of input_to_output's ``raw`` tensor (lvd.py:846) and returned as a strided
    (B*Tc*Tp -> B, Tc, Tp, L, Hd, Wd) view of it.  ``channels`` = C of the frames that will be warped,
    ``include_self``: whether ``raw`` gets the extra self context.  Returns (flow, alpha_ctx view (B, Tc, Tp, L,
    Hd, Wd), disocc, amax or None, slots): ``slots`` (a ``RawSlots``) goes to ``frame_warp_fuse_raw``.
    ``raw_dtype``: the element type ``raw`` is allocated in -- fp32, or bf16 / fp16 for a UNet under autocast: the alpha
    slots (and later the warped channels) are the fp32 values rounded to nearest-even, ``.to(raw_dtype)``'s bits; flow,
    disocc, amax and the score stay fp32."""
    if raw_dtype not in _DTYPE_CODE:
        raise _lib.WaldoHipError(f"flow_ctx_warp_into_raw: raw_dtype must be fp32, bf16 or fp16, got {raw_dtype}")
    if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (flow_lr, a01, occ)):
        raise _lib.WaldoHipError("flow_ctx_warp_into_raw: no gradient flows through the raw-slot path; use flow_ctx_warp")
    flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ = _flow_ctx_warp_args("flow_ctx_warp_into_raw", flow_lr, isobj_lr, a01,
                                                                       ctx_ts, pred_ts, occ, tw, scale)
    nl = flow_lr.shape[1]
    b, tc, tp = ctx_ts.shape
    hd, wd = a01.shape[-2:]
    tcx = tc + (1 if include_self else 0)
    st, strict = _status(status)
    with torch.no_grad():
        raw = flow_lr.new_empty(b, tp, tcx, channels + nl, hd, wd, dtype=raw_dtype)
        score = flow_lr.new_empty(b, tc, tp, hd, wd)
        name, codes = _dt_entry("waldo_flow_ctx_warp_raw_fwd", raw_dtype)
        flow, disocc, amax = _flow_ctx_warp_fwd(name, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, tw, scale, layer_max,
                                                st.ptr, _layer_bits_ptr("flow_ctx_warp_into_raw", layer_bits, a01),
                                                (raw, score), int(channels), tcx, *codes)
        alpha_ctx = raw[:, :, :tc, channels:].permute(0, 2, 1, 3, 4, 5)  # (B, Tc, Tp, L, Hd, Wd), strided
    if strict:
        st.check(sync=True)
    return flow, alpha_ctx, disocc, amax, RawSlots(raw, score, int(channels), bool(include_self))


MAX_FUSE_CTX = 8


class _FrameWarpFuse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, flow, alpha, ctx_ts, include_self, eps, status_ptr):
        b, t, c, hd, wd = input.shape
        _, tc, tp, nl = alpha.shape[:4]
        tcx = tc + (1 if include_self else 0)
        out = input.new_empty(b, tp, c + 1, hd, wd)
        # stored (B, Tp, Tc', ...) and handed out as the reference's (B, Tc', Tp, ...) VIEW: WIF.forward's
        # permute(0, 2, 1, ...).contiguous() (wif.py:39) then is a no-op instead of a copy of the
        # pipeline's largest tensor (C4 recipe: 11.8 GB read + written per predict)
        raw = input.new_empty(b, tp, tcx, c + nl, hd, wd)
        _lib.launch("waldo_frame_warp_fuse_fwd", input.device, input, flow, alpha, ctx_ts, out, raw, status_ptr, b, t, tc,
                    tp, c, nl, hd, wd, 1 if include_self else 0, float(eps))
        ctx.save_for_backward(input, flow, alpha, ctx_ts)
        ctx.cfg = (bool(include_self), float(eps))
        # an output the loss does not use comes back as None, not as a zero-filled tensor of its size (raw_output is
        # the largest tensor of the chain; the kernel takes NULL for either gradient)
        ctx.set_materialize_grads(False)
        return out, raw.permute(0, 2, 1, 3, 4, 5)

    @staticmethod
    def backward(ctx, g_out, g_raw):
        input, flow, alpha, ctx_ts = ctx.saved_tensors
        include_self, eps = ctx.cfg
        b, t, c, hd, wd = input.shape
        _, tc, tp, nl = alpha.shape[:4]
        g_out = _c(g_out) if g_out is not None else None
        g_raw = _c(g_raw) if g_raw is not None else None
        g_flow = torch.empty_like(flow)
        g_alpha = torch.empty_like(alpha)
        _lib.launch("waldo_frame_warp_fuse_bwd", input.device, input, flow, alpha, ctx_ts, g_out, g_raw, g_flow, g_alpha,
                    b, t, tc, tp, c, nl, hd, wd, 1 if include_self else 0, eps)
        return None, g_flow, g_alpha, None, None, None, None


def frame_warp_fuse(input, flow, alpha, ctx_ts, include_self=False, eps=1e-6, status=None):
    """Warper.input_to_output (models/nets/lvd.py:830-853).  input (B,T,C,Hd,Wd);
    flow (B,Tc,Tp,2,Hd,Wd); alpha (B,Tc,Tp,L,Hd,Wd) in [-1,1]; ctx_ts (B,Tc,Tp) long.
    Returns (out (B,Tp,C+1,Hd,Wd), raw (B,Tc',Tp,C+L,Hd,Wd)).  Differentiable w.r.t. flow and alpha;
    the frames in ``input`` are data (no gradient is produced for them).  ``ctx_ts`` must lie in [0, T): validated
    on the device (``status``: see ``flow_ctx_warp``)."""
    _lib.check_cuda(input, flow, alpha)
    if not ctx_ts.is_cuda:
        raise _lib.WaldoHipError("frame_warp_fuse: ctx_ts must be on the GPU")
    input, flow = _c(input.detach()), _c(flow)
    ctx_ts = _c(ctx_ts.long())
    b, t, c, hd, wd = input.shape
    _, tc, tp, nl = alpha.shape[:4]
    if tuple(flow.shape) != (b, tc, tp, 2, hd, wd) or tuple(alpha.shape) != (b, tc, tp, nl, hd, wd) \
            or tuple(ctx_ts.shape) != (b, tc, tp):
        raise _lib.WaldoHipError(
            f"frame_warp_fuse: inconsistent shapes input={tuple(input.shape)} flow={tuple(flow.shape)} "
            f"alpha={tuple(alpha.shape)} ctx_ts={tuple(ctx_ts.shape)}")
    st, strict = _status(status)
    res = _FrameWarpFuse.apply(input, flow, _c(alpha), ctx_ts, bool(include_self), eps, st.ptr)
    if strict:
        st.check(sync=True)
    return res


def frame_warp_fuse_raw(input, flow, slots, ctx_ts, eps=1e-6, status=None):
    """``frame_warp_fuse`` behind ``flow_ctx_warp_into_raw`` (no autograd): the context alphas already sit in
    ``slots.raw`` and their per-context sums in ``slots.score``, so they are neither read nor copied -- one score
    plane per context instead of L alpha planes.  The same bits as ``frame_warp_fuse`` on the alpha view
    (tests/test_gpu_warper.py::test_alpha_ctx_written_into_raw_slots).  Returns (out, raw as (B, Tc', Tp, ...)).
    A 16-bit ``slots.raw`` (``flow_ctx_warp_into_raw(..., raw_dtype=...)``) gets the warped channels rounded to
    nearest-even; ``out`` is fp32 either way.  ``input`` may be a ``PackedClip``: the same bits as on its unpacked form
    (``waldo_frame_warp_fuse_raw_packed_fwd``: one word per tap for all channels)."""
    packed = isinstance(input, PackedClip)
    _lib.check_cuda(flow, *(() if packed else (input,)))
    if not ctx_ts.is_cuda:
        raise _lib.WaldoHipError("frame_warp_fuse_raw: ctx_ts must be on the GPU")
    if torch.is_grad_enabled() and flow.requires_grad:
        raise _lib.WaldoHipError("frame_warp_fuse_raw: no gradient flows through the raw-slot path; use frame_warp_fuse")
    input, flow = (input if packed else _c(input.detach())), _c(flow.detach())
    ctx_ts = _c(ctx_ts.long())
    b, t, c, hd, wd = input.shape
    raw, score = slots.raw, slots.score
    _, tc, tp = score.shape[:3]
    nl = raw.shape[3] - c
    tcx = tc + (1 if slots.include_self else 0)
    if slots.channels != c or tuple(raw.shape) != (b, tp, tcx, c + nl, hd, wd) or tuple(score.shape) != (b, tc, tp, hd, wd) \
            or tuple(flow.shape) != (b, tc, tp, 2, hd, wd) or tuple(ctx_ts.shape) != (b, tc, tp):
        raise _lib.WaldoHipError(
            f"frame_warp_fuse_raw: inconsistent shapes input={tuple(input.shape)} flow={tuple(flow.shape)} "
            f"raw={tuple(raw.shape)} score={tuple(score.shape)} ctx_ts={tuple(ctx_ts.shape)}")
    st, strict = _status(status)
    out = input.new_empty(b, tp, c + 1, hd, wd)
    with torch.no_grad():
        if packed:
            _lib.launch("waldo_frame_warp_fuse_raw_packed_fwd", input.device, _packed_data(input, "frame_warp_fuse_raw"),
                        rgb_table(input.device), flow, score, ctx_ts, out, raw, st.ptr, b, t, tc, tp, input.num_lyt, nl,
                        hd, wd, 1 if slots.include_self else 0, float(eps), _DTYPE_CODE[raw.dtype])
        else:
            name, codes = _dt_entry("waldo_frame_warp_fuse_raw_fwd", raw.dtype)
            _lib.launch(name, input.device, input, flow, score, ctx_ts, out, raw, st.ptr, b, t, tc, tp, c, nl, hd, wd,
                        1 if slots.include_self else 0, float(eps), *codes)
    if strict:
        st.check(sync=True)
    return out, raw.permute(0, 2, 1, 3, 4, 5)


# --------------------------------------------------------------------------------------
# The packed clip: (B, T, Hd, Wd) pixels of 4 bytes [R, G, B, class id] in place of the (B, T, 3 + Nl, Hd, Wd) fp32 clip
# --------------------------------------------------------------------------------------
MAX_PACKED_LYT = 32  # layout classes of a packed clip (the fused path's limit, include/waldo_hip.h "Packed clip")
_RGB_TABLES = {}


def rgb_table(device):
    """The 256 fp32 values of read_rgb's normalisation (``tools.io.rgb_from_u8`` of every byte), built on the host as
    ``read_rgb`` computes them and kept once per device."""
    key = str(device)
    if key not in _RGB_TABLES:
        from .tools.io import rgb_from_u8
        _RGB_TABLES[key] = rgb_from_u8(torch.arange(256, dtype=torch.uint8)).to(device)
    return _RGB_TABLES[key]


class PackedClip:
    """A clip as ``data`` (B, T, Hd, Wd, 4) uint8, bytes [R, G, B, class id] per pixel: what a user loads from 8-bit PNG
    frames and class maps, 4 bytes per pixel where the fp32 clip takes 4 (3 + ``num_lyt``).  It stands for its UNPACKED
    form (B, T, 3 + num_lyt, Hd, Wd) fp32 (``unpack()``): channels 0-2 the ``rgb_table`` entries of the RGB bytes
    (``tools.io.read_rgb``), channel 3 + n +5 where the class id is n and -5 elsewhere (``tools.io.read_layout``; a class
    id >= num_lyt: -5 in every layout channel).

    ``Warper`` / ``decode_output`` take it wherever they take the fp32 clip, with the same results bit for bit: on the
    fused path without autograd the packed kernels read it (no fp32 copy is made), every other path unpacks it once.
    It offers what that code reads of a clip -- ``shape`` / ``size()`` of the unpacked form, ``device``, slicing along
    batch and time (views), ``new_empty`` (fp32, as the unpacked clip's) -- and carries no gradient."""

    __slots__ = ("data", "num_lyt")
    ndim = 5
    dtype = torch.float32  # (of the unpacked form)
    requires_grad = False

    def __init__(self, data, num_lyt):
        num_lyt = int(num_lyt)
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.ndim != 5 or data.shape[-1] != 4:
            raise ValueError(f"PackedClip: data must be a (B, T, Hd, Wd, 4) uint8 tensor, got "
                             f"{getattr(data, 'dtype', type(data))} {tuple(getattr(data, 'shape', ()))}")
        if not 0 <= num_lyt <= MAX_PACKED_LYT:
            raise ValueError(f"PackedClip: num_lyt {num_lyt} outside [0, {MAX_PACKED_LYT}]")
        self.data, self.num_lyt = data, num_lyt

    @property
    def shape(self):
        b, t, hd, wd, _ = self.data.shape
        return torch.Size((b, t, 3 + self.num_lyt, hd, wd))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 5

    @property
    def device(self):
        return self.data.device

    @property
    def is_cuda(self):
        return self.data.is_cuda

    @property
    def _version(self):  # (tools.demo.SharedContext keys on identity + version)
        return self.data._version

    def is_inference(self):
        return self.data.is_inference()

    def __getitem__(self, idx):
        """Batch and time slices (views): ``clip[b0:b1]``, ``clip[:, t0:t1]``."""
        idx = idx if isinstance(idx, tuple) else (idx,)
        if len(idx) > 2 or not all(isinstance(i, slice) for i in idx):
            raise IndexError("PackedClip: only slices along batch and time (clip[b0:b1, t0:t1]); unpack() for more")
        return PackedClip(self.data[idx], self.num_lyt)

    def to(self, device, non_blocking=False):
        return PackedClip(self.data.to(device, non_blocking=non_blocking), self.num_lyt)

    def new_empty(self, *size, dtype=torch.float32):
        """An uninitialised tensor on the clip's device, fp32 like the unpacked clip's ``new_empty``."""
        return torch.empty(*size, dtype=dtype, device=self.device)

    def unpack(self):
        """The unpacked fp32 clip (B, T, 3 + num_lyt, Hd, Wd): one ``waldo_unpack_clip_fwd`` launch."""
        return unpack_clip(self)

    def rgb(self):
        """Channels 0-2 of the unpacked clip alone (B, T, 3, Hd, Wd): the same launch without the layout planes."""
        return unpack_clip(PackedClip(self.data, 0))

    def __repr__(self):
        return f"PackedClip(shape={tuple(self.shape)}, num_lyt={self.num_lyt}, device={self.device})"


def pack_clip(rgb_u8, class_ids, num_lyt):
    """A ``PackedClip`` from tensors the caller holds: ``rgb_u8`` (B, T, 3, Hd, Wd) uint8 and ``class_ids`` (B, T, Hd, Wd)
    integer class ids in [0, 255] (ids >= num_lyt stand for all-(-5) layout logits).  Data preparation (torch ops);
    the result lives on ``rgb_u8``'s device."""
    if not torch.is_tensor(rgb_u8) or rgb_u8.dtype != torch.uint8 or rgb_u8.ndim != 5 or rgb_u8.shape[2] != 3:
        raise ValueError(f"pack_clip: rgb_u8 must be (B, T, 3, Hd, Wd) uint8, got {getattr(rgb_u8, 'dtype', None)} "
                         f"{tuple(getattr(rgb_u8, 'shape', ()))}")
    b, t, _, hd, wd = rgb_u8.shape
    if tuple(class_ids.shape) != (b, t, hd, wd) or class_ids.is_floating_point() or class_ids.is_complex():
        raise ValueError(f"pack_clip: class_ids must be integer (B, T, Hd, Wd) = {(b, t, hd, wd)}, got "
                         f"{class_ids.dtype} {tuple(class_ids.shape)}")
    if class_ids.dtype != torch.uint8 and class_ids.numel() and (int(class_ids.min()) < 0 or int(class_ids.max()) > 255):
        raise ValueError("pack_clip: class ids outside [0, 255] do not fit a byte")
    cls = class_ids.to(device=rgb_u8.device, dtype=torch.uint8)
    return PackedClip(torch.cat([rgb_u8.permute(0, 1, 3, 4, 2), cls.unsqueeze(-1)], dim=-1).contiguous(), num_lyt)


def _packed_data(clip, fn):
    if not clip.is_cuda:
        raise _lib.WaldoHipError(f"{fn}: the packed clip must be on the GPU (PackedClip.to(device)); there is no CPU "
                                 "fallback")
    return _c(clip.data)


def unpack_clip(clip):
    """``PackedClip`` -> its unpacked form (B, T, 3 + Nl, Hd, Wd) fp32 (``waldo_unpack_clip_fwd``)."""
    data = _packed_data(clip, "unpack_clip")
    b, t, hd, wd, _ = data.shape
    out = torch.empty(clip.shape, dtype=torch.float32, device=data.device)
    _lib.launch("waldo_unpack_clip_fwd", data.device, data, rgb_table(data.device), out, b, t, clip.num_lyt, hd, wd)
    return out


# --------------------------------------------------------------------------------------
# Byte output (include/waldo_hip.h "Byte output"): predicted frames as uint8, quantised on the device
# --------------------------------------------------------------------------------------
BYTE_QUANTIZE = {"trunc": 0, "round": 1}  # WALDO_METRICS_TRUNC / _ROUND
BYTE_LAYOUT = {"nchw": 0, "nhwc": 1}  # WALDO_BYTES_NCHW / _NHWC
_SRC_PACKED = 3  # WALDO_BYTES_SRC_PACKED


def _f32(v):
    return ctypes.c_float(v).value


def _byte_args(fn, span, quantize, layout):
    """(lo, range, quantisation code, layout code); range = hi - lo in fp32, as the header defines it."""
    if quantize not in BYTE_QUANTIZE:
        raise ValueError(f"{fn}: quantize must be one of {tuple(BYTE_QUANTIZE)}, got {quantize!r}")
    if layout not in BYTE_LAYOUT:
        raise ValueError(f"{fn}: layout must be one of {tuple(BYTE_LAYOUT)}, got {layout!r}")
    lo, hi = (_f32(float(v)) for v in span)
    if not hi > lo:
        raise ValueError(f"{fn}: span {tuple(span)} must have lo < hi")
    return lo, _f32(hi - lo), BYTE_QUANTIZE[quantize], BYTE_LAYOUT[layout]


def _dense_tail(t, k):
    """Whether the last ``k`` dimensions of ``t`` are laid out densely (a dimension of size 1 may have any stride)."""
    expect = 1
    for d in range(t.ndim - 1, t.ndim - 1 - k, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            return False
        expect *= t.shape[d]
    return True


def _flat_frames(d):
    """(..., C, H, W) as (N, C, H, W) with W unit-stride: a view where the strides allow it, one copy otherwise."""
    c, h, w = d.shape[-3:]
    if d.stride(-1) != 1 and w > 1:
        d = d.contiguous()
    return d.reshape(-1, c, h, w)


def _check_out(fn, out, lead, frame, name="out"):
    """``out=`` of a byte output, where given: a uint8 tensor of the result's shape."""
    if out is None:
        return
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (*lead, *frame):
        raise ValueError(f"{fn}: {name} must be a uint8 tensor of shape {(*lead, *frame)}, got "
                         f"{getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))}")


def _dest(fn, out, n, frame, device, name="out"):
    """The (n, *frame) destination of a byte output: a new tensor, or ``out`` (past ``_check_out``) viewed so -- dense
    frames, leading dimensions flattened by stride, any alignment."""
    if out is None:
        return torch.empty((n, *frame), dtype=torch.uint8, device=device)
    if out.device != device:
        raise ValueError(f"{fn}: the input on {device}, {name} on {out.device}")
    try:
        o = out.view(n, *frame)
    except RuntimeError:
        o = None
    if o is None or not _dense_tail(o, len(frame)):
        raise ValueError(f"{fn}: {name} must hold dense frames whose leading dimensions flatten by stride "
                         f"(strides {tuple(out.stride())})")
    return o


def _frame_stride(o, frame_bytes):
    """The stride between the frames of ``o``; of one frame alone, its size (the stride of a dimension of 1 is free)."""
    return o.stride(0) if o.shape[0] > 1 else frame_bytes


def frames_to_bytes(x, span=(-1.0, 1.0), quantize="trunc", layout="nchw", out=None):
    """Frames as bytes (``waldo_frames_to_bytes_fwd``): with ``u = clamp((x - lo) / (hi - lo), 0, 1)`` in fp32,
    ``"trunc"``: ``uint8(trunc(u * 255))``, what the reference's ``dump_video`` writes (tools/utils.py:246-264);
    ``"round"``: ``uint8(trunc(u * 255 + 0.5))``, what ``tools.io.dump_video`` / ``dump_image`` write.  NaN gives 0.
    These are the bytes ``metrics.frame_metrics`` scores under the same ``quantize``.

    ``x``: a tensor (..., C, H, W) in fp32, bf16 or fp16 (W unit-stride; the leading dimensions are flattened by stride
    where that is possible -- ``output[:, :, :3]`` is read in place -- and copied once otherwise), or a ``PackedClip``
    (its three RGB channels: the quantised ``rgb_table`` values of its bytes, which under ``"trunc"`` are NOT its bytes
    for 63 of the 256 values).  ``layout``: ``"nchw"`` -> uint8 (..., C, H, W); ``"nhwc"`` -> uint8 (..., H, W, 3), what a
    video writer takes (C must be 3).  ``out``: a uint8 tensor of the result's shape to write into -- each frame dense,
    the leading dimensions flattenable by stride, any alignment (a view into a larger buffer).
    Detached: no gradient flows, nothing is registered with autograd.  No CPU fallback."""
    fn = "frames_to_bytes"
    lo, rng, quant, lay = _byte_args(fn, span, quantize, layout)
    if isinstance(x, PackedClip):
        d = _packed_data_view(x, fn)
        lead, (h, w), c = tuple(d.shape[:2]), d.shape[2:4], 3
        d = d.flatten(0, 1)  # (a view where the strides allow it)
        code, strides, table = _SRC_PACKED, (d.stride(0) // 4, 0, d.stride(1) // 4), rgb_table(d.device)
    else:
        if not torch.is_tensor(x) or x.ndim < 3 or x.dtype not in _DTYPE_CODE:
            raise ValueError(f"{fn}: x must be a (..., C, H, W) float32 / bfloat16 / float16 tensor or a PackedClip, got "
                             f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
        if not x.is_cuda:
            raise _lib.WaldoHipError(f"{fn}: x must be on the GPU (cuda device); there is no CPU fallback")
        d = x.detach()
        lead, (c, h, w) = tuple(d.shape[:-3]), d.shape[-3:]
        if min(c, h, w) < 1:
            raise ValueError(f"{fn}: empty frames {tuple(x.shape)}")
        d = _flat_frames(d)
        code, strides, table = _DTYPE_CODE[d.dtype], (d.stride(0), d.stride(1), d.stride(2)), None
    if lay and c != 3:
        raise ValueError(f"{fn}: layout 'nhwc' takes 3 channels, got {c}")
    n = d.shape[0]
    frame = (h, w, 3) if lay else (c, h, w)
    _check_out(fn, out, lead, frame)
    o = _dest(fn, out, n, frame, d.device)
    _lib.launch("waldo_frames_to_bytes_fwd", d.device, d, code, *strides, table, o, _frame_stride(o, c * h * w), lay, n,
                c, h, w, lo, rng, quant)
    return out if out is not None else o.view(*lead, *frame)


def _packed_data_view(clip, fn):
    """A packed clip's bytes as the kernels address them: 4-byte pixels at 4-byte aligned, pixel-multiple strides."""
    if not clip.is_cuda:
        raise _lib.WaldoHipError(f"{fn}: the packed clip must be on the GPU (PackedClip.to(device)); there is no CPU "
                                 "fallback")
    d = clip.data
    if d.stride(-1) != 1 or d.stride(-2) != 4 or d.data_ptr() % 4 or any(d.stride(i) % 4 for i in range(3)):
        d = d.contiguous()
    return d


def wif_fuse_bytes(vid, net_out, ab=True, span=(-1.0, 1.0), quantize="trunc", layout="nchw"):
    """``frames_to_bytes(wif_fuse(vid, net_out, ab), span, quantize, layout)`` in ONE launch
    (``waldo_wif_fuse_bytes_fwd``): the same bytes, without the fp32 frames in between.  uint8 (B, T, 3, H, W) or, with
    ``layout="nhwc"``, (B, T, H, W, 3).  Forward only: raises when grad mode is on and an input requires a gradient."""
    fn = "wif_fuse_bytes"
    lo, rng, quant, lay = _byte_args(fn, span, quantize, layout)
    _lib.check_cuda(vid, net_out, half=True)
    if torch.is_grad_enabled() and (vid.requires_grad or net_out.requires_grad):
        raise _lib.WaldoHipError(f"{fn}: no gradient flows through the byte output; use wif_fuse")
    vid, net = _c(vid.detach()), _c(net_out.detach())
    b, t, tc, c, h, w = vid.shape
    co = net.shape[3]
    if tuple(net.shape) != (b, t, tc, co, h, w):
        raise _lib.WaldoHipError(f"{fn}: shapes {tuple(vid.shape)} vs {tuple(net.shape)}")
    out = torch.empty((b, t, h, w, 3) if lay else (b, t, 3, h, w), dtype=torch.uint8, device=vid.device)
    name, codes = _dt_entry("waldo_wif_fuse_bytes_fwd", vid.dtype, net.dtype)
    _lib.launch(name, vid.device, vid, net, out, b * t, tc, c, co, h * w, int(bool(ab)), lo, rng, quant, lay, *codes)
    return out


# --------------------------------------------------------------------------------------
# A8: gather_time and the frame arithmetic built on it
# --------------------------------------------------------------------------------------
class _TimeGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ctx_ts, pred_ts, tc, hw, subtract, status_ptr):
        b, t = x.shape[:2]
        p = math.prod(x.shape[2:]) // 2
        tp = pred_ts.numel()
        out = x.new_empty(b, tc, tp, *((p // hw, 2, hw) if hw else (p, 2)))
        _lib.launch("waldo_time_gather_fwd", x.device, x, ctx_ts, pred_ts, out, status_ptr, b, t, tc, tp, p, hw,
                    int(subtract))
        ctx.save_for_backward(ctx_ts, pred_ts)
        ctx.cfg = (tuple(x.shape), tc, hw, subtract)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ctx_ts, pred_ts = ctx.saved_tensors
        shape, tc, hw, subtract = ctx.cfg
        grad_out = _c(grad_out)
        gx = grad_out.new_empty(shape)
        b, t = shape[:2]
        _lib.launch("waldo_time_gather_bwd", grad_out.device, grad_out, ctx_ts, pred_ts, gx, b, t, tc, pred_ts.numel(),
                    math.prod(shape[2:]) // 2, hw, int(subtract))
        return gx, None, None, None, None, None, None


def time_gather(x, ctx_ts, pred_ts, num_ctx=None, subtract=False, channel_first=False, status=None):
    """``gather_time`` (models/nets/lvd.py:462-467) and the frame arithmetic of the flow synthesis
    (lvd.py:660-668, 780-787) on a clip's grids ``x`` (B, T, ..., 2):

    - ``subtract``: ``gather_time(x, ctx_ts) - x[:, pred_ts].unsqueeze(1)``            -> (B, Tc, Tp, ..., 2)
    - ``ctx_ts is None``: ``x[:, pred_ts].unsqueeze(1).expand(-1, num_ctx, ...)``     -> (B, num_ctx, Tp, ..., 2)
    - otherwise ``gather_time(x, ctx_ts)``.

    ``channel_first``: x is (B, T, N, H, W, 2) and the result (B, Tc, Tp, N, 2, H, W) -- the
    ``permute(0, 1, 2, 3, 6, 4, 5)`` of lvd.py:662.  Differentiable w.r.t. ``x``.  Frame indices must lie in [0, T):
    validated on the device (``status``: see ``flow_ctx_warp``).  For ONE context and a ``pred_ts`` made by
    ``arange_index(T)`` the result is a VIEW of ``x`` (see there)."""
    _lib.check_cuda(x)
    if x.ndim < 3 or x.shape[-1] != 2 or (channel_first and x.ndim != 6):
        raise _lib.WaldoHipError(f"time_gather: x {tuple(x.shape)} is not a clip of grids (B, T, ..., 2)")
    if not pred_ts.is_cuda or (ctx_ts is not None and not ctx_ts.is_cuda):
        raise _lib.WaldoHipError("time_gather: frame indices must be on the GPU")
    x = _c(x.float())
    pred_ts = _c(pred_ts.long())
    b, t = x.shape[:2]
    if ctx_ts is not None:
        ctx_ts = _c(ctx_ts.long())
        if ctx_ts.ndim != 3 or ctx_ts.shape[0] != b or ctx_ts.shape[2] != pred_ts.numel():
            raise _lib.WaldoHipError(f"time_gather: ctx_ts {tuple(ctx_ts.shape)} against B={b}, Tp={pred_ts.numel()}")
        tc = ctx_ts.shape[1]
    else:
        if subtract or num_ctx is None:
            raise _lib.WaldoHipError("time_gather: without ctx_ts give num_ctx (and no difference)")
        tc = int(num_ctx)
    tp = pred_ts.numel()
    if ctx_ts is None and tc == 1 and tp == t and not channel_first and _is_arange_index(pred_ts):
        # x[:, [0, 1, ..., T - 1]] for one context: the clip itself (a view: no copy, and the backward is autograd's sum
        # instead of a scatter kernel) -- the LVD recipe's `ctx_mode "prev"`, where every frame is predicted
        return x.view(b, 1, t, *x.shape[2:])
    hw = x.shape[3] * x.shape[4] if channel_first else 0
    st, strict = _status(status)
    out = _TimeGather.apply(x, ctx_ts, pred_ts, tc, hw, bool(subtract), st.ptr)
    if strict:
        st.check(sync=True)
    if channel_first:
        return out.view(b, tc, tp, x.shape[2], 2, x.shape[3], x.shape[4])
    return out.view(b, tc, tp, *x.shape[2:])


def downscale_frames(input, num_frames, first_channel, factor):
    """``scale(input[:, :num_frames, first_channel:], 1 / factor)`` of ``Warper.grid_to_flow[_ctx]``
    (models/nets/lvd.py:611 / 716): the low-resolution copy of the layout channels, the same bits as
    ``F.interpolate(..., scale_factor=1 / factor, mode="bilinear")`` on the device for a power-of-two ``factor``.
    The frames are data: the result carries no gradient.  A ``PackedClip`` (``first_channel`` 3: its layout channels)
    gives the bits of its unpacked form (``waldo_downscale_frames_packed_fwd``: one read of each pixel's word)."""
    packed = isinstance(input, PackedClip)
    if not packed:
        _lib.check_cuda(input)
    b, t, c, hd, wd = input.shape
    s = int(factor)
    if s < 2 or s & (s - 1) or hd % s or wd % s:
        raise _lib.WaldoHipError(f"downscale_frames: factor {factor} on {hd} x {wd} frames (a power of two that divides both)")
    if packed:
        if int(first_channel) != 3:
            raise _lib.WaldoHipError(f"downscale_frames: a packed clip's layout channels start at 3, not {first_channel}")
        data = _packed_data(input, "downscale_frames")
        out = torch.empty(b, int(num_frames), c - 3, hd // s, wd // s, device=data.device)
        _lib.launch("waldo_downscale_frames_packed_fwd", data.device, data, out, b, t, int(num_frames), c - 3, hd // s,
                    wd // s, s)
        return out
    x = _c(input.detach().float())
    out = x.new_empty(b, int(num_frames), c - int(first_channel), hd // s, wd // s)
    _lib.launch("waldo_downscale_frames_fwd", x.device, x, out, b, t, int(num_frames), c, int(first_channel), hd // s,
                wd // s, s)
    return out


def points_in_polygon(pts, corners, valid=None):
    """``matplotlib.path.Path(corners).contains_points(pts)`` (radius 0, no transform) on the device, as ``WIF.inpaint``
    uses it (models/nets/wif.py:228-235): ``pts`` (..., 2) float32 (x, y) on the GPU, ``corners`` a sequence of 3 ... 16
    (x, y) pairs of host numbers -> a bool tensor of ``pts.shape[:-1]``.  matplotlib's crossings test in double precision,
    operation by operation: points on an edge get matplotlib's answer.

    ``corners`` may also be a tensor ON THE DEVICE (nothing is read on the host): (K, 2) -> ``pts.shape[:-1]``, or
    (P, K, 2), P polygons tested against the same points -> (P, *pts.shape[:-1]); float64 (float32 is widened
    exactly).  ``valid`` (P,) on the device, any integer or bool type: a polygon whose entry is zero contains nothing."""
    _lib.check_cuda(pts)
    if pts.shape[-1] != 2:
        raise _lib.WaldoHipError(f"points_in_polygon: points of shape {tuple(pts.shape)} (..., 2)")
    if torch.is_tensor(corners):
        return _points_in_polygon_dev(pts, corners, valid)
    if valid is not None:
        raise _lib.WaldoHipError("points_in_polygon: `valid` goes with corners on the device")
    flat = [float(v) for c in corners for v in c]
    k = len(flat) // 2
    if len(flat) != 2 * k or any(len(c) != 2 for c in corners) or k > 16:
        raise _lib.WaldoHipError(f"points_in_polygon: {len(corners)} corners (pairs, at most 16)")
    host = (ctypes.c_double * max(len(flat), 1))(*flat)
    x = _c(pts.detach())
    n = x.numel() // 2
    out = x.new_empty(x.shape[:-1])
    _lib.launch("waldo_points_in_polygon_fwd", x.device, x, ctypes.addressof(host), k, out, n)
    return out > 0


def _polygon_regions(pts, corners, valid):
    """The device form of the polygon test as 0 / 1 floats: ``corners`` (P, K, 2) float64 and ``valid`` (P,) int32 or
    None, both on the device and taken by their strides (a side of ``border_objects``' tables is read in place) ->
    (P, *pts.shape[:-1]) float32."""
    if not corners.is_cuda or corners.dim() != 3 or corners.shape[2] != 2 or corners.shape[1] > 16:
        raise _lib.WaldoHipError(f"points_in_polygon: device corners of shape {tuple(corners.shape)} ((P, K, 2) on the "
                                 "GPU, at most 16 corners)")
    p, k = corners.shape[:2]
    cn = corners.detach().to(torch.float64)
    if k and (cn.stride(2) != 1 or cn.stride(1) != 2 or cn.stride(0) < 0):
        cn = cn.contiguous()
    if valid is not None:
        if not valid.is_cuda or tuple(valid.shape) != (p,):
            raise _lib.WaldoHipError(f"points_in_polygon: `valid` of shape {tuple(valid.shape)} for {p} polygons on the GPU")
        valid = valid.detach()
        if valid.dtype != torch.int32 or valid.stride(0) < 0:
            valid = (valid != 0).to(torch.int32)
    x = _c(pts.detach())
    n = x.numel() // 2
    out = x.new_empty((p,) + tuple(x.shape[:-1]))
    _lib.launch("waldo_points_in_polygon_dev_fwd", x.device, x, cn, cn.stride(0) if p and k else 0, valid,
                valid.stride(0) if valid is not None else 0, k, out, p, n)
    return out


def _points_in_polygon_dev(pts, corners, valid):
    if corners.dim() == 2:
        if valid is not None:
            valid = valid.reshape(1)
        return _polygon_regions(pts, corners.unsqueeze(0), valid)[0] > 0
    return _polygon_regions(pts, corners, valid) > 0


def border_objects(pred_flow, ident, alpha_ctx):
    """The border objects of ``WIF.inpaint`` (models/nets/wif.py:134-157) for every clip of a batch, chosen on the
    device (csrc/border_objects.hip): ``pred_flow`` (B, 2, H, W), the flow of the last context to the last predicted
    frame in grid units (any strides over B and the channel: ``pred_flow[:, -1, -1]`` is read in place), ``ident``
    (H, W, 2) the identity grid, ``alpha_ctx`` (B, Tc, Tp, L, H, W) in [-1, 1] (any strides over the first four
    dimensions) -> ``(valid (B, 2) int32, obj_id (B, 2) int64, corners (B, 2, 4, 2) float64)``, side 0 = left, 1 = right.
    No host read; the values have the bits of the torch expressions evaluated per clip."""
    _lib.check_cuda(pred_flow, ident, alpha_ctx)
    if alpha_ctx.dim() != 6 or pred_flow.dim() != 4:
        raise _lib.WaldoHipError(f"border_objects: alpha_ctx of shape {tuple(alpha_ctx.shape)} (B, Tc, Tp, L, H, W), "
                                 f"pred_flow of shape {tuple(pred_flow.shape)} (B, 2, H, W)")
    b, tc, tp, nl, h, w = alpha_ctx.shape
    if tuple(pred_flow.shape) != (b, 2, h, w) or ident.numel() != h * w * 2 or ident.shape[-1] != 2:
        raise _lib.WaldoHipError(f"border_objects: pred_flow {tuple(pred_flow.shape)}, identity grid {tuple(ident.shape)} "
                                 f"for {b} clips of {h} x {w}")
    if not 2 <= nl <= 32 or tc < 1 or tp < 1:
        raise _lib.WaldoHipError(f"border_objects: {nl} layers, {tc} contexts, {tp} predicted frames (2 ... 32 layers)")
    x, f, ident = alpha_ctx.detach(), pred_flow.detach(), _c(ident.detach())
    if x.stride(5) != 1 or x.stride(4) != w or min(x.stride()[:4]) < 0:
        x = x.contiguous()
    if f.stride(3) != 1 or f.stride(2) != w or min(f.stride()[:2]) < 0:
        f = f.contiguous()
    dev = x.device
    valid = torch.empty(b, 2, dtype=torch.int32, device=dev)
    obj_id = torch.empty(b, 2, dtype=torch.int64, device=dev)
    corners = torch.empty(b, 2, 4, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(max(_lib.query("waldo_border_objects_workspace_bytes", b) // 4, 1), dtype=torch.int32, device=dev)
    _lib.launch("waldo_border_objects_fwd", dev, f, f.stride(0), f.stride(1), ident, x, x.stride(0), x.stride(1),
                x.stride(2), x.stride(3), valid, obj_id, corners, ws, b, tc, tp, nl, h, w)
    return valid, obj_id, corners


def inpaint_propagate(flow, ident, ref_img, ref_mask, shadow, entering, img, todo, obj, soft_shadow=False,
                      fix_mask=False):
    """One frame of the propagation loop of ``WIF.inpaint`` (models/nets/wif.py:179-211) in one launch -- the warps of
    the reference background, its mask and the shadow mask by ``flow + ident``, the entering objects
    (``entering``: up to two ``(region, look, flow_k)``), the fill of the frame's holes and the inpainter's inputs --
    with the bits of the spelled-out composition.  Returns ``(img, todo, inpainter_img, inpainter_mask)``; with
    ``fix_mask`` the inpainter takes ``img`` itself and ``inpainter_mask`` is the undilated ``1 - (1 - todo)(1 - obj)``."""
    _lib.check_cuda(flow, ident, ref_img, ref_mask, shadow, img, todo, obj)
    b, c, h, w = img.shape
    if c != 3 or len(entering) > 2:
        raise _lib.WaldoHipError(f"inpaint_propagate: {c} channels, {len(entering)} entering objects (3; at most 2)")
    flow, ident, ref_img, ref_mask, img, todo, obj = (_c(x.detach()) for x in (flow, ident, ref_img, ref_mask, img, todo, obj))
    shadow = _c(shadow.detach()) if shadow is not None else None
    for x, shape in ((flow, (b, h, w, 2)), (ref_img, (b, 3, h, w)), (ref_mask, (b, 1, h, w)), (todo, (b, 1, h, w)),
                     (obj, (b, 1, h, w))) + (((shadow, (b, 1, h, w)),) if shadow is not None else ()):
        if tuple(x.shape) != shape:
            raise _lib.WaldoHipError(f"inpaint_propagate: a tensor of shape {tuple(x.shape)} where {shape} is expected")
    if ident.numel() != h * w * 2:
        raise _lib.WaldoHipError(f"inpaint_propagate: an identity grid of shape {tuple(ident.shape)} for {h} x {w} frames")
    keep = []  # (contiguous copies must outlive the launch's enqueue)
    ptrs = [[], [], []]
    for region, look, fk in entering:
        _lib.check_cuda(region, look, fk)
        region, look, fk = _c(region.detach().expand(b, 1, h, w)), _c(look.detach()), _c(fk.detach())
        if tuple(look.shape) != (b, 3, h, w) or tuple(fk.shape) != (b, h, w, 2):
            raise _lib.WaldoHipError("inpaint_propagate: an entering object's look / flow has the wrong shape")
        keep += [region, look, fk]
        for lst, x in zip(ptrs, (region, look, fk)):
            lst.append(x.data_ptr())
    arrs = [(ctypes.c_void_p * 2)(*(lst + [None] * (2 - len(lst)))) for lst in ptrs]
    img_out, todo_out, inp_mask = torch.empty_like(img), torch.empty_like(todo), torch.empty_like(todo)
    inp_img = None if fix_mask else torch.empty_like(img)
    _lib.launch("waldo_inpaint_propagate_fwd", img.device, flow, ident, ref_img, ref_mask, shadow,
                ctypes.addressof(arrs[0]), ctypes.addressof(arrs[1]), ctypes.addressof(arrs[2]), len(entering), img, todo,
                obj, img_out, todo_out, inp_img, inp_mask, b, h, w, int(bool(soft_shadow)), int(bool(fix_mask)))
    return img_out, todo_out, (img_out if fix_mask else inp_img), inp_mask


def inpaint_holes(alpha_ctx, last_only=False, fix_thresh=True):
    """The hole and object masks of ``WIF.inpaint`` (models/nets/wif.py:60-75) from ``alpha_ctx`` (B, Tc, Tp, L, H, W)
    in [-1, 1] in ONE pass (any strides over the first four dimensions: the raw-slot view of ``decode_output`` is taken
    as it is): ``(mask, obj_mask)``, each (B, Tp, 1, H, W) of 0 / 1 -- before the optional expansion of wif.py:76-77.
    The sums over the layers are taken in the order of the framework's reduction: the same mask pixels."""
    _lib.check_cuda(alpha_ctx)
    if alpha_ctx.dim() != 6:
        raise _lib.WaldoHipError(f"inpaint_holes: alpha_ctx of shape {tuple(alpha_ctx.shape)} (B, Tc, Tp, L, H, W)")
    x = alpha_ctx.detach()
    b, tc, tp, nl, h, w = x.shape
    if x.stride(5) != 1 or x.stride(4) != w or min(x.stride()[:4]) < 0:
        x = x.contiguous()
    mask = x.new_empty(b, tp, 1, h, w)
    obj_mask = x.new_empty(b, tp, 1, h, w)
    _lib.launch("waldo_inpaint_holes_fwd", x.device, x, x.stride(0), x.stride(1), x.stride(2), x.stride(3), mask,
                obj_mask, b, tc, tp, nl, h * w, int(bool(last_only)), 0.1 if fix_thresh else 0.9)
    return mask, obj_mask


def inpaint_blend(img, todo, fill):
    """``(1 - todo) * img + todo * fill`` (wif.py:214) in one launch; img / fill (B, 3, H, W), todo (B, 1, H, W)."""
    _lib.check_cuda(img, todo, fill)
    img, todo, fill = _c(img.detach()), _c(todo.detach()), _c(fill.detach())
    b, c, h, w = img.shape
    if c != 3 or tuple(fill.shape) != tuple(img.shape) or tuple(todo.shape) != (b, 1, h, w):
        raise _lib.WaldoHipError(f"inpaint_blend: shapes {tuple(img.shape)}, {tuple(todo.shape)}, {tuple(fill.shape)}")
    out = torch.empty_like(img)
    _lib.launch("waldo_inpaint_blend_fwd", img.device, img, todo, fill, out, b, h * w)
    return out


_EXPAND_STEPS = {None: 15, "": 15, "south": 1, "north": 2, "east": 4, "west": 8}


def mask_expand(mask, num=1, dir=None, soft=False, alpha=0.97):
    """The reference's ``expand`` (tools/utils.py:300-323) as ONE launch: ``num`` rounds of one-pixel growth towards
    the south, north, east and west in that order along dims 2 and 3 of ``mask``, each step seeing the one before
    (``dir`` keeps one of the four); hard masks (``soft=False``) are read as ``mask != 0`` and returned as float
    0 / 1, soft ones grow by ``max(pixel, alpha * neighbour)``.  The same bits as the framework's 8 * num launches
    (``waldo_amd.tools.utils.expand`` states them) for every input; never writes its argument.

    ``mask``: (N, C, H, W) -- or, as ``WIF.inpaint`` calls it on its (B, Tp, 1, H, W) hole masks (wif.py:77), five
    dimensions of which dim 2 has size 1: dims 2 and 3 are then (1, H), so "south / north" have nothing to do and "east /
    west" run along H -- the reference's own behaviour, kept."""
    if not mask.is_cuda:
        raise _lib.WaldoHipError("waldo_amd ops need tensors on the GPU (cuda device); there is no CPU fallback")
    if dir not in _EXPAND_STEPS:
        raise ValueError(f"mask_expand: dir {dir!r} (south, north, east, west or None)")
    steps = _EXPAND_STEPS[dir]
    if mask.dim() == 4:
        planes, h, w = mask.shape[0] * mask.shape[1], mask.shape[2], mask.shape[3]
    elif mask.dim() == 5 and mask.shape[2] == 1:
        # dims (2, 3) = (1, H) with W elementwise behind them: east / west of the reference run along H = the kernel's
        # south / north on (H, W) planes; its south / north see a dimension of size 1
        planes, h, w = mask.shape[0] * mask.shape[1], mask.shape[3], mask.shape[4]
        steps = ((steps >> 2) & 3)
    else:
        raise _lib.WaldoHipError(f"mask_expand: a mask of shape {tuple(mask.shape)} (four dimensions, or five with a "
                                 f"dim 2 of size 1)")
    if soft and mask.dtype != torch.float32:
        raise _lib.WaldoHipError(f"mask_expand: a soft mask of dtype {mask.dtype} (float32: the kernel's arithmetic)")
    x = _c(mask.detach().float())
    num = int(num)
    if num == 0 or steps == 0 or planes == 0:
        return x.clone() if soft else (x != 0).float()
    out = torch.empty_like(x)
    scratch = torch.empty_like(x) if num > 30 else None
    _lib.launch("waldo_mask_expand_fwd", x.device, x, out, scratch, planes, h, w, num, steps, 1 if soft else 0,
                float(alpha))
    return out


# --------------------------------------------------------------------------------------
# fused hot path
# --------------------------------------------------------------------------------------
class _WarpComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layers, mapping, occ, basis_t, want_alpha, delta):
        _lib.check_cuda(layers, half=True)  # (a 16-bit stack: warp_composite() sends only served shapes here)
        _lib.check_cuda(mapping, occ, basis_t)
        layers, mapping, occ, basis_t = _c(layers), _c(mapping), _c(occ), _c(basis_t)
        f, nl, c, h, w = layers.shape
        if c != 4:
            raise _lib.WaldoHipError("warp_composite expects (F, L, 4, H, W) layers (RGB + alpha)")
        k3 = mapping.shape[1]
        if mapping.shape[0] != f * nl or tuple(occ.shape) != (f, nl, nl) or \
                tuple(basis_t.shape) != (k3, h * w):
            raise _lib.WaldoHipError(
                f"warp_composite: inconsistent shapes layers={tuple(layers.shape)} "
                f"mapping={tuple(mapping.shape)} occ={tuple(occ.shape)} basis_t={tuple(basis_t.shape)}")
        rgb = layers.new_empty(f, 3, h, w, dtype=torch.float32)
        alpha = layers.new_empty(f, nl, h, w, dtype=torch.float32) if want_alpha else None
        name, codes = _dt_entry("waldo_warp_composite_fwd", layers.dtype)
        _lib.launch(name, layers.device, layers, basis_t, mapping, occ, rgb, alpha, f, nl, h, w, k3, float(delta), *codes)
        ctx.save_for_backward(layers, mapping, occ, basis_t)
        ctx.want_alpha = want_alpha
        ctx.delta = float(delta)
        ctx.det = is_deterministic()
        if ctx.det and any(ctx.needs_input_grad[:3]) and f > 0 and \
                _lib.query("waldo_warp_composite_bwd_det_workspace_bytes", f, nl, h, w, k3) <= 0:
            raise _det_unserved("warp_composite", f"L = {nl}, K3 = {k3}, W = {w}: the generic backward sums with float "
                                "atomics; the two-kernel backward needs L <= 17, K3 == 19 and 4 | W")
        return rgb, alpha

    @staticmethod
    def backward(ctx, grad_rgb, grad_alpha):
        layers, mapping, occ, basis_t = ctx.saved_tensors
        f, nl, _, h, w = layers.shape
        k3 = mapping.shape[1]
        grad_rgb = _c(grad_rgb)
        if grad_alpha is not None:
            grad_alpha = _c(grad_alpha)
        summed = (mapping if ctx.needs_input_grad[1] else None, occ if ctx.needs_input_grad[2] else None)
        if ctx.det:  # (every gradient overwritten; the dtype code travels in every case)
            gm, go = _empty_like_each(*summed)
            gl = torch.empty_like(layers)
            if f == 0:
                return gl, gm, go, None, None, None
            ws, ws_bytes = _det_workspace("warp_composite", "waldo_warp_composite_bwd_det_workspace_bytes",
                                          (f, nl, h, w, k3), layers.device)
            name, codes = "waldo_warp_composite_bwd_det", (_DTYPE_CODE[layers.dtype],)
        else:
            gm, go = _zeros_like_each(*summed)
            # 0: the shape is served by the generic kernel (or a test asked for it: WALDO_DEBUG_BWD_GENERIC)
            ws_bytes = _lib.query("waldo_warp_composite_bwd_workspace_bytes", f, nl, h, w, k3)
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=layers.device) if ws_bytes else None
            # with a workspace the two-kernel path writes every texel of grad_layers exactly once;
            # the generic kernel accumulates with atomics into a zero-filled buffer.  (A 16-bit stack: grad_layers in
            # its type, from the two-kernel path only.)
            gl = torch.empty_like(layers) if ws_bytes else torch.zeros_like(layers)
            name, codes = _dt_entry("waldo_warp_composite_bwd", layers.dtype)
        _lib.launch(name, layers.device, layers, basis_t, mapping, occ, grad_rgb, grad_alpha, gl, gm, go, ws, ws_bytes, f,
                    nl, h, w, k3, ctx.delta, *codes)
        return gl, gm, go, None, None, None


def warp_composite(layers, src_pts, occ, inverse_kernel, basis_t, return_alpha=False, delta=0.0):
    """Fused TPS grid -> bilinear warp of each 4-channel layer -> LVD.reduce_comp
    (models/modules/warp.py:49-55, F.grid_sample, models/nets/lvd.py:100-114).

    layers (F, L, 4, H, W) in [-1, 1]; src_pts (F*L, N, 2); occ (F, L, L);
    inverse_kernel (N+3, N+3); basis_t (N+3, H*W).  Returns rgb (F, 3, H, W) and, if asked,
    the composited alpha (F, L, H, W), both in [-1, 1].

    delta: the layers are sampled as ``F.grid_sample(x + delta, grid) - delta`` (lvd.py:548,559).
    0 (default) is the BASELINE pipeline of SURVEY 8d: taps outside a layer contribute 0 (alpha 0.5 /
    grey after ``reduce_comp``'s ``(x + 1) / 2``); 1 is ``Warper.layer_to_output``'s default:
    out-of-range taps read -1, i.e. alpha 0 / black.  Precision / NaN contract of the backward:
    include/waldo_hip.h.

    ``layers`` may be fp16 or bf16 (a decoder under autocast); every other operand stays fp32.  The kernels widen
    each texel exactly: rgb and alpha (fp32) have the bits of the call on ``layers.float()``, and the gradient of
    ``layers`` comes back in its type, the fp32 gradient rounded to nearest-even.  Shapes the 16-bit kernels do not
    serve (``_layers16_served``) run the fp32 path on ``layers.float()`` inside the autograd graph, which keeps the
    same contract."""
    f, nl = layers.shape[:2]
    needs_grad = torch.is_grad_enabled() and any(
        torch.is_tensor(t) and t.requires_grad for t in (layers, src_pts, occ, inverse_kernel, basis_t))
    if layers.dtype in (torch.float16, torch.bfloat16) and not _layers16_served(layers, src_pts, needs_grad):
        return warp_composite(layers.float(), src_pts, occ, inverse_kernel, basis_t, return_alpha, delta)
    # the one-launch forward pays for its launch saving with a mapping computation per (tile, frame):
    # worth it while the call is launch-bound (C2: 25 -> 19 us), 4 % slower at C4 size
    small = f * ((layers.shape[-2] + 15) // 16) * ((layers.shape[-1] + 15) // 16) <= FOLD_MAX_TILE_FRAMES
    if not needs_grad and small and layers.dim() == 5 and layers.shape[2] == 4 and src_pts.dim() == 3 and \
            _lib.load().waldo_warp_composite_pts_supported(nl, layers.shape[-2], layers.shape[-1],
                                                           src_pts.shape[1]):
        return _warp_composite_pts(layers, src_pts, occ, inverse_kernel, basis_t, bool(return_alpha),
                                   float(delta))
    mapping = tps_mapping(inverse_kernel, src_pts)
    chunk = _frames_per_call(f, nl, layers.shape[-2], layers.shape[-1], mapping.shape[1])
    if f <= chunk:
        rgb, alpha = _WarpComposite.apply(layers, mapping, occ, basis_t, bool(return_alpha), float(delta))
    else:  # frames are independent: long batches go in pieces (launch limits, bounded workspace)
        outs = [_WarpComposite.apply(layers[i:i + chunk], mapping[i * nl:(i + chunk) * nl], occ[i:i + chunk],
                                     basis_t, bool(return_alpha), float(delta)) for i in range(0, f, chunk)]
        rgb = torch.cat([o[0] for o in outs])
        alpha = torch.cat([o[1] for o in outs]) if return_alpha else None
    return (rgb, alpha) if return_alpha else rgb


def _layers16_served(layers, src_pts, needs_grad):
    """A 16-bit layer stack runs on its own kernels: the staged forward (waldo_warp_composite_pts_supported) and, with
    a gradient, the two-kernel backward (a workspace size > 0).  Both queries honour the debug options."""
    if layers.dim() != 5 or layers.shape[2] != 4 or src_pts.dim() != 3:
        return False
    f, nl, _, h, w = layers.shape
    lib = _lib.load()
    n = src_pts.shape[1]
    if nl < 1 or not lib.waldo_warp_composite_pts_supported(nl, h, w, n):
        return False
    return not needs_grad or _lib.query("waldo_warp_composite_bwd_workspace_bytes", max(f, 1), nl, h, w, n + 3) > 0


def _warp_composite_pts(layers, src_pts, occ, inverse_kernel, basis_t, want_alpha, delta):
    """Forward without autograd, straight from the control points: ONE launch per call
    (waldo_warp_composite_pts_fwd; the TPS mapping is computed inside the kernel, same bits as
    tps_mapping + the two-step forward)."""
    _lib.check_cuda(layers, half=True)
    _lib.check_cuda(src_pts, occ, inverse_kernel, basis_t)
    layers, src_pts, occ = _c(layers.detach()), _c(src_pts.detach().float()), _c(occ.detach())
    inverse_kernel, basis_t = _c(inverse_kernel.detach()), _c(basis_t.detach())
    f, nl, _, h, w = layers.shape
    n = src_pts.shape[1]
    if src_pts.shape[0] != f * nl or tuple(occ.shape) != (f, nl, nl) or \
            tuple(basis_t.shape) != (n + 3, h * w) or tuple(inverse_kernel.shape) != (n + 3, n + 3):
        raise _lib.WaldoHipError(
            f"warp_composite: inconsistent shapes layers={tuple(layers.shape)} src_pts={tuple(src_pts.shape)} "
            f"occ={tuple(occ.shape)} basis_t={tuple(basis_t.shape)} inverse_kernel={tuple(inverse_kernel.shape)}")
    rgb = layers.new_empty(f, 3, h, w, dtype=torch.float32)
    alpha = layers.new_empty(f, nl, h, w, dtype=torch.float32) if want_alpha else None
    per = max(1, MAX_FL_PER_LAUNCH // nl)
    name, codes = _dt_entry("waldo_warp_composite_pts_fwd", layers.dtype)
    for i in range(0, f, per):
        j = min(f, i + per)
        _lib.launch(name, layers.device, layers[i:j], basis_t, inverse_kernel, src_pts[i * nl:j * nl], occ[i:j], rgb[i:j],
                    alpha[i:j] if want_alpha else None, j - i, nl, h, w, n, delta, *codes)
    return (rgb, alpha) if want_alpha else rgb


FOLD_MAX_TILE_FRAMES = 8192     # largest (frames x 16x16 tiles) the one-launch forward is used for
MAX_WORKSPACE_BYTES = 8 << 30   # backward workspace per call of the fused path
MAX_FL_PER_LAUNCH = 65535       # F * L limit of one launch (include/waldo_hip.h)


def _frames_per_call(f, nl, h, w, k3):
    """Largest number of frames one call of the fused path may take."""
    if f == 0:
        return 1
    per = max(1, MAX_FL_PER_LAUNCH // nl)
    ws1, ws8 = (_lib.query("waldo_warp_composite_bwd_workspace_bytes", n, nl, h, w, k3) for n in (1, 8))
    per_frame = max((ws8 - ws1) / 7.0, 1.0) if ws8 > 0 else 0.0
    if per_frame:
        per = min(per, max(1, int(MAX_WORKSPACE_BYTES // per_frame)))
    return per


# --------------------------------------------------------------------------------------
# plane norm + GELU (+ the concatenation with a skip): what lies between the UNet's convolutions
# --------------------------------------------------------------------------------------
# The launcher's gate: with a gradient required, planes whose H W lies in one of these ranges (lo, hi),
# inclusive, take the framework ops although the tensors are on the GPU -- the level shapes where tools_dev/ab_unet.py
# measured forward + backward of the op slower than GroupNorm + GELU + cat (a few megabytes per call: the time is the
# host's, and the autograd node of a Python op costs more of it than three framework nodes).  Forward without
# autograd: the kernel at every shape.
PLANE_NORM_GRAD_FRAMEWORK_HW = ((1, 512),)           # with a skip to concatenate: the decoder's 16 x 32 level
PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP = ((1, 8192),)  # without: the encoder's 8 x 16 to 64 x 128 levels


def plane_norm_limits():
    """The launcher's regime boundaries in H W, ascending (``waldo_plane_norm_limits``): planes of at most ``[0]``
    values take a wavefront each, up to ``[-1]`` a workgroup each, larger ones are cut into chunks of ``[-1]``."""
    buf = (ctypes.c_int * 8)()
    n = _lib.load().waldo_plane_norm_limits(buf, 8)
    return [int(buf[i]) for i in range(n)]


def plane_norm_gelu_framework(x, weight, bias, skip=None, eps=1e-5):
    """``plane_norm_gelu`` spelled out in framework ops, as the reference runs it (models/modules/conv.py:19-25, 59):
    GroupNorm with one group per channel, the exact GELU, ``torch.cat`` with the skip.  The CPU route of
    ``plane_norm_gelu`` and the ``fused = False`` route of ``modules.UNet``."""
    # (torch.group_norm itself: F.group_norm first refuses N H W == 1, which is a legal plane here -- z = beta)
    y = torch.nn.functional.gelu(torch.group_norm(x, x.shape[1], weight, bias, eps, torch.backends.cudnn.enabled))
    return y if skip is None else torch.cat([y, skip], dim=1)


def _dense_planes(t):
    """``t`` (N, C, H, W) with every (n, c) plane dense -- any batch and channel stride: itself, else a dense copy."""
    if t.is_contiguous():
        return t
    h, w = t.shape[2:]
    if (w == 1 or t.stride(3) == 1) and (h == 1 or t.stride(2) == w):
        return t
    return t.contiguous()


_plane_norm_chunk = None


def _plane_norm_workspace(x):
    """(buffer or None, bytes): what ``waldo_plane_norm_workspace_bytes`` returns for x's shape -- two floats per chunk
    of a plane above the last regime boundary, nothing below -- worked out here from the limits (queried once): the
    host's work per call is what a small level costs."""
    global _plane_norm_chunk
    if _plane_norm_chunk is None:
        _plane_norm_chunk = plane_norm_limits()[-1]
    n, c, h, w = x.shape
    if h * w <= _plane_norm_chunk:
        return None, 0
    words = n * c * (-(-h * w // _plane_norm_chunk)) * 2
    return torch.empty(words, dtype=torch.float32, device=x.device), words * 4


_PLANE_NORM_16BIT = (torch.bfloat16, torch.float16)


class _PlaneNormGelu(torch.autograd.Function):
    """x, skip and the output (backward: x, grad_out, grad_x) of ONE element type -- fp32, or bf16 / fp16 through the
    ``_dt`` entry points; weight, bias, the statistics and the workspace fp32 whatever it is."""

    @staticmethod
    def forward(ctx, x, weight, bias, skip, eps):
        _lib.check_cuda(x, skip, half=True)
        _lib.check_cuda(weight, bias)
        n, c, h, w = x.shape
        x, weight, bias = _dense_planes(x), _c(weight), _c(bias)
        cs = ss_n = ss_c = 0
        if skip is not None:
            if skip.dtype != x.dtype:
                raise _lib.WaldoHipError(f"plane_norm_gelu: x is {x.dtype} and skip is {skip.dtype}")
            skip = _dense_planes(skip)
            cs, ss_n, ss_c = skip.shape[1], skip.stride(0), skip.stride(1)
        out = x.new_empty(n, c + cs, h, w)
        stats = torch.empty(2, n * c, dtype=torch.float32, device=x.device)  # mean, rstd
        ws, nbytes = _plane_norm_workspace(x)
        args = (x, x.stride(0), x.stride(1), weight, bias, float(eps), skip, ss_n, ss_c, out, (c + cs) * h * w, stats,
                stats.data_ptr() + 4 * n * c, ws, nbytes, n, c, cs, h, w)
        if x.dtype == torch.float32:
            _lib.launch("waldo_plane_norm_gelu_fwd", x.device, *args)
        else:
            _lib.launch("waldo_plane_norm_gelu_fwd_dt", x.device, *args, _DTYPE_CODE[x.dtype])
        ctx.save_for_backward(x, weight, bias, stats)
        ctx.has_skip = skip is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, weight, bias, stats = ctx.saved_tensors
        n, c, h, w = x.shape
        gx = gw = gb = gs = None
        if grad_out.dtype != x.dtype:
            grad_out = grad_out.to(x.dtype)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            grad_out = _dense_planes(grad_out)  # (its first C channels are read through the strides: no copy)
            gx = x.new_empty(n, c, h, w)
            sums = torch.empty(n, c, 2, dtype=torch.float32, device=x.device)
            ws, nbytes = _plane_norm_workspace(x)
            args = (x, x.stride(0), x.stride(1), weight, bias, stats, stats.data_ptr() + 4 * n * c, grad_out,
                    grad_out.stride(0), grad_out.stride(1), gx, sums, ws, nbytes, n, c, h, w)
            if x.dtype == torch.float32:
                _lib.launch("waldo_plane_norm_gelu_bwd", x.device, *args)
            else:
                _lib.launch("waldo_plane_norm_gelu_bwd_dt", x.device, *args, _DTYPE_CODE[x.dtype])
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                # (over n: a framework reduction with a fixed order, no atomics)
                gb, gw = (sums[0] if n == 1 else sums.sum(dim=0)).unbind(1)
        if ctx.has_skip and ctx.needs_input_grad[3]:
            gs = grad_out[:, c:]
        return gx, gw, gb, gs, None


def plane_norm_gelu(x, weight, bias, skip=None, eps=1e-5, out_dtype=None):
    """``cat([gelu(group_norm(x, C, weight, bias, eps)), skip], dim=1)`` -- one UNet level's work between two
    convolutions (include/waldo_hip.h "Plane norm") as one op: x (N, C, H, W), weight / bias (C), skip (N, Cs, H, W) or
    None -> (N, C + Cs, H, W).  Differentiable in x, weight, bias and skip; keeps x and two floats per plane for the
    backward, which is free of atomics (the same bits from run to run in either deterministic mode).  Tensors on the
    CPU take the same arithmetic in framework ops (``plane_norm_gelu_framework``), as do, under autograd, the planes of
    ``PLANE_NORM_GRAD_FRAMEWORK_HW`` (``_NO_SKIP``).

    ``out_dtype=None``: fp32; under autocast the inputs are cast to fp32, as ``group_norm``'s are, and the result is
    fp32.  A bf16 / fp16 ``x`` on the GPU outside autocast runs as ``out_dtype=x.dtype``.

    ``out_dtype=torch.bfloat16 | torch.float16`` (a UNet under autocast: ``modules.UNet.act_dtype``): x, skip and the
    result are STORED in that type, with or without autocast around the call (it is disabled inside; the casts carry
    the gradients).  The kernel widens on load, keeps fp32 statistics, registers and sums, and rounds once to
    nearest-even on the store -- the values the next convolution under autocast would round the fp32 result to; the
    skip slice is ``skip``'s bits.  ``x`` and ``skip`` of another type are cast to ``out_dtype`` first: the statistics
    are then those of the ROUNDED values, which is what a convolution under autocast hands over.  ``weight`` and
    ``bias`` are used in fp32.  ``grad_x`` and ``grad_skip`` come back in the 16-bit type, ``grad_weight`` and
    ``grad_bias`` in fp32; the backward keeps the 16-bit x: half the bytes.  The CPU route and the gated planes compute
    ``plane_norm_gelu_framework`` on fp32 copies and cast the result.  Any other ``out_dtype``: ValueError."""
    if out_dtype is not None and out_dtype not in _PLANE_NORM_16BIT:
        raise ValueError(f"plane_norm_gelu: out_dtype must be None, torch.bfloat16 or torch.float16, got {out_dtype!r}")
    if x.dim() != 4:
        raise ValueError(f"plane_norm_gelu: x must be (N, C, H, W), got {tuple(x.shape)}")
    n, c, h, w = x.shape
    if tuple(weight.shape) != (c,) or tuple(bias.shape) != (c,):
        raise ValueError(f"plane_norm_gelu: weight and bias must be ({c},), got {tuple(weight.shape)}, {tuple(bias.shape)}")
    if skip is not None and (skip.dim() != 4 or skip.shape[0] != n or tuple(skip.shape[2:]) != (h, w)):
        raise ValueError(f"plane_norm_gelu: skip must be ({n}, Cs, {h}, {w}), got {tuple(skip.shape)}")
    kernel = x.is_cuda and x.numel() != 0
    if kernel:
        gate = PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP if skip is None else PLANE_NORM_GRAD_FRAMEWORK_HW
        kernel = not (gate and any(lo <= h * w <= hi for lo, hi in gate) and torch.is_grad_enabled() and
                      (x.requires_grad or weight.requires_grad or bias.requires_grad
                       or (skip is not None and skip.requires_grad)))
    if out_dtype is None and x.is_cuda and x.dtype in _PLANE_NORM_16BIT and not torch.is_autocast_enabled("cuda"):
        out_dtype = x.dtype
    if out_dtype is not None:
        with torch.autocast(x.device.type, enabled=False):
            x, weight, bias = x.to(out_dtype), weight.float(), bias.float()
            skip = None if skip is None else skip.to(out_dtype)
            if kernel:
                return _PlaneNormGelu.apply(x, weight, bias, skip, eps)
            return plane_norm_gelu_framework(x.float(), weight, bias, None if skip is None else skip.float(),
                                             eps).to(out_dtype)
    if not kernel:
        return plane_norm_gelu_framework(x, weight, bias, skip, eps)
    if torch.is_autocast_enabled("cuda"):  # fp32 inside, as group_norm: the casts carry the gradients back
        with torch.autocast("cuda", enabled=False):
            return _PlaneNormGelu.apply(x.float(), weight.float(), bias.float(), None if skip is None else skip.float(),
                                        eps)
    return _PlaneNormGelu.apply(x, weight, bias, skip, eps)


# --------------------------------------------------------------------------------------
# token attention: softmax(scale q k^T) v over one or two key / value segments (the LVD transformer blocks)
# --------------------------------------------------------------------------------------
_token_attention_limits_read = {}


def _token_attention_limits_of(symbol):
    """``{"q_tile", "k_tile", "head_dims"}`` as the library's ``symbol`` reports them (read once per symbol)."""
    if symbol not in _token_attention_limits_read:
        buf = (ctypes.c_int * 16)()
        n = getattr(_lib.load(), symbol)(buf, 16)
        vals = [int(buf[i]) for i in range(n)]
        _token_attention_limits_read[symbol] = {"q_tile": vals[0], "k_tile": vals[1], "head_dims": tuple(vals[2:])}
    return dict(_token_attention_limits_read[symbol])


def token_attention_limits():
    """``{"q_tile", "k_tile", "head_dims"}`` of the kernel (``waldo_token_attention_limits``): query rows per
    workgroup, keys per LDS tile, the head dimensions it serves."""
    return _token_attention_limits_of("waldo_token_attention_limits")


def _token_attention_check(q, k, v, k2, v2):
    if q.dim() != 4:
        raise ValueError(f"token_attention: q must be (B, Nq, H, D), got {tuple(q.shape)}")
    b, _, h, d = q.shape
    if k.dim() != 4 or k.shape[0] != b or tuple(k.shape[2:]) != (h, d) or k.shape[1] < 1 or v.shape != k.shape:
        raise ValueError(f"token_attention: k and v must be ({b}, Nk >= 1, {h}, {d}), got {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    if (k2 is None) != (v2 is None):
        raise ValueError("token_attention: k2 and v2 come together")
    if k2 is not None and (k2.dim() != 4 or k2.shape[0] != b or tuple(k2.shape[2:]) != (h, d) or v2.shape != k2.shape):
        raise ValueError(f"token_attention: k2 and v2 must be ({b}, Nk2, {h}, {d}), got {tuple(k2.shape)}, "
                         f"{tuple(v2.shape)}")


def token_attention_framework(q, k, v, k2=None, v2=None, scale=None):
    """``token_attention`` spelled out in framework ops, as the reference runs it (models/modules/transform.py:109-117
    for one segment, :175-185 for two): matmul, scale, ``cat`` of the two score blocks, softmax, ``cat`` of the values,
    matmul, transpose, reshape.  The CPU route of ``token_attention``, the ``fused = False`` route of the transformer
    blocks and what the ``"framework"`` backward route of the kernel differentiates."""
    _token_attention_check(q, k, v, k2, v2)
    b, nq, h, d = q.shape
    scale = d ** -0.5 if scale is None else scale
    qh, vh = q.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    attn = (qh @ k.permute(0, 2, 3, 1)) * scale
    if k2 is not None:
        attn = torch.cat([attn, (qh @ k2.permute(0, 2, 3, 1)) * scale], dim=-1)
        vh = torch.cat([vh, v2.permute(0, 2, 1, 3)], dim=2)
    attn = attn.softmax(dim=-1)
    return (attn @ vh).transpose(1, 2).reshape(b, nq, h * d)


def _token_view_strides(t):
    """(batch stride, token stride) of a (B, N, H, D) view whose (token, head) rows are D consecutive floats D apart
    and start on 16-byte boundaries -- what ``waldo_token_attention_fwd`` reads in place -- else None.  (The stride of
    an axis of one element is free.)"""
    b, n, h, d = t.shape
    if (d > 1 and t.stride(3) != 1) or (h > 1 and t.stride(2) != d) or t.data_ptr() % 16:
        return None
    sb, sn = (t.stride(0) if b > 1 else 0), (t.stride(1) if n > 1 else 0)
    if sb % 4 or sn % 4 or sb < 0 or sn < 0:
        return None
    return sb, sn


def _token_attention_served(q, k, v, k2, v2):
    """The strides of the operands if the kernel serves them as they lie, else None."""
    ts = [t for t in (q, k, v, k2, v2) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == q.device for t in ts):
        return None
    if q.shape[3] not in token_attention_limits()["head_dims"] or q.numel() == 0:
        return None
    if k2 is not None and k2.shape[1] == 0:
        return None
    if torch.is_autocast_enabled("cuda"):
        return None
    strides = [_token_view_strides(t) for t in ts]
    return None if any(s is None for s in strides) else strides


def token_attention_bwd_limits():
    """``token_attention_limits`` of the backward's kernels (``waldo_token_attention_bwd_limits``): ``q_tile`` the query
    rows per workgroup of the dQ kernel and per LDS tile of the dK/dV kernel, ``k_tile`` the keys per LDS tile of the dQ
    kernel and per workgroup of the dK/dV kernel."""
    return _token_attention_limits_of("waldo_token_attention_bwd_limits")


TOKEN_ATTENTION_BACKWARD_ROUTES = ("kernel", "framework")
_token_attention_backward_route = "framework"


def get_token_attention_backward_route():
    """The route the backward of a ``token_attention`` whose forward runs now will take."""
    return _token_attention_backward_route


class token_attention_backward_route:
    """``token_attention_backward_route(route)`` sets how the kernel route of ``token_attention`` differentiates:
    ``"kernel"`` -- ``waldo_token_attention_bwd`` from the forward's ``out`` and row statistics (no score tensor, no
    atomics) -- or ``"framework"`` -- ``token_attention_framework`` recomputed from the saved views and differentiated
    (kept for A/B runs and as the fallback).  Used as ``with token_attention_backward_route(route):`` the earlier setting
    comes back on exit, also after an exception; nests.  The route is read when the op's FORWARD runs and travels with
    the autograd node.  The default is ``"framework"`` (the measurements favour the kernel; the default
    follows once the launch counts the suite pins for a training step change with it)."""

    def __init__(self, route):
        global _token_attention_backward_route
        if route not in TOKEN_ATTENTION_BACKWARD_ROUTES:
            raise ValueError(f"token_attention_backward_route: route must be one of {TOKEN_ATTENTION_BACKWARD_ROUTES}, "
                             f"got {route!r}")
        self.route = route
        self.prev = _token_attention_backward_route
        _token_attention_backward_route = route

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _token_attention_backward_route
        _token_attention_backward_route = self.prev
        return False


TOKEN_ATTENTION_16BIT_ROUTES = ("framework", "kernel")
_token_attention_16bit_route = "framework"


def get_token_attention_16bit_route():
    """The route ``token_attention`` / ``token_attention_clips`` take on bf16 / fp16 operands now."""
    return _token_attention_16bit_route


class token_attention_16bit_route:
    """``token_attention_16bit_route(route)`` sets what ``token_attention`` and ``token_attention_clips`` do with bf16 /
    fp16 operands on the GPU: ``"framework"`` (the default) -- ``token_attention_framework`` /
    ``token_attention_clips_framework``, as before there was a 16-bit kernel -- or ``"kernel"`` --
    ``waldo_token_attention_fwd_dt`` / ``waldo_token_attention_clips_fwd_dt`` where the operands meet the layout rules
    (``_token_attention_served_16bit``), also while autocast is enabled.  fp32 operands are not touched by the switch.
    Used as ``with token_attention_16bit_route(route):`` the earlier setting comes back on exit, also after an
    exception; nests.  The route is read when the op's forward runs."""

    def __init__(self, route):
        global _token_attention_16bit_route
        if route not in TOKEN_ATTENTION_16BIT_ROUTES:
            raise ValueError(f"token_attention_16bit_route: route must be one of {TOKEN_ATTENTION_16BIT_ROUTES}, "
                             f"got {route!r}")
        self.route = route
        self.prev = _token_attention_16bit_route
        _token_attention_16bit_route = route

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _token_attention_16bit_route
        _token_attention_16bit_route = self.prev
        return False


TOKEN_ATTENTION_16BIT_BACKWARD_ROUTES = ("framework", "kernel")
_token_attention_16bit_backward_route = "framework"


def get_token_attention_16bit_backward_route():
    """The route the backward of a 16-bit kernel ``token_attention`` whose forward runs now will take."""
    return _token_attention_16bit_backward_route


class token_attention_16bit_backward_route:
    """``token_attention_16bit_backward_route(route)`` sets how a ``token_attention`` call that the 16-bit kernel serves
    (bf16 / fp16 operands under ``token_attention_16bit_route("kernel")``) differentiates: ``"framework"`` (the
    default) -- ``token_attention_framework`` recomputed from the saved views and differentiated, as before there was a
    16-bit backward -- or ``"kernel"`` -- the forward runs ``waldo_token_attention_fwd_lse_dt`` and saves ``out`` and
    ``lse`` with the views, and ONE ``waldo_token_attention_bwd_dt`` call computes only the wanted gradients (no score
    tensor, no atomics).  A switch of its own: ``token_attention_backward_route`` does not reach 16-bit calls.  It has
    no effect on the CPU, on fp32 operands, under the default 16-bit route and on ``token_attention_clips`` (whose
    16-bit backward stays the recompute).  Used as ``with token_attention_16bit_backward_route(route):`` the earlier
    setting comes back on exit, also after an exception; nests.  The route is read when the op's FORWARD runs and
    travels with the autograd node."""

    def __init__(self, route):
        global _token_attention_16bit_backward_route
        if route not in TOKEN_ATTENTION_16BIT_BACKWARD_ROUTES:
            raise ValueError(f"token_attention_16bit_backward_route: route must be one of "
                             f"{TOKEN_ATTENTION_16BIT_BACKWARD_ROUTES}, got {route!r}")
        self.route = route
        self.prev = _token_attention_16bit_backward_route
        _token_attention_16bit_backward_route = route

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _token_attention_16bit_backward_route
        _token_attention_16bit_backward_route = self.prev
        return False


def token_attention_16bit_limits():
    """``token_attention_limits`` of the 16-bit kernels (``waldo_token_attention_dt_limits``)."""
    return _token_attention_limits_of("waldo_token_attention_dt_limits")


def _same_16bit_on_gpu(ts):
    return ts[0].dtype in (torch.float16, torch.bfloat16) and all(
        t.is_cuda and t.dtype == ts[0].dtype and t.device == ts[0].device for t in ts)


def _token_view_strides_16bit(t):
    """``_token_view_strides`` for 16-bit rows: strides in elements, multiples of 8 (16-byte pieces)."""
    b, n, h, d = t.shape
    if (d > 1 and t.stride(3) != 1) or (h > 1 and t.stride(2) != d) or t.data_ptr() % 16:
        return None
    sb, sn = (t.stride(0) if b > 1 else 0), (t.stride(1) if n > 1 else 0)
    if sb % 8 or sn % 8 or sb < 0 or sn < 0:
        return None
    return sb, sn


def _token_attention_served_16bit(q, k, v, k2, v2):
    """The strides of the operands if the 16-bit kernel serves them as they lie under the route set now, else None:
    bf16 or fp16 tensors of one type on one GPU, the route ``"kernel"``, D in the kernel's head dimensions, a unit inner
    stride, heads D apart, rows on 16-byte boundaries.  Autocast does not matter: the operands already are 16-bit."""
    if _token_attention_16bit_route != "kernel":
        return None
    ts = [t for t in (q, k, v, k2, v2) if t is not None]
    if not _same_16bit_on_gpu(ts):
        return None
    if q.shape[3] not in token_attention_16bit_limits()["head_dims"] or q.numel() == 0:
        return None
    if k2 is not None and k2.shape[1] == 0:
        return None
    strides = [_token_view_strides_16bit(t) for t in ts]
    return None if any(s is None for s in strides) else strides


class _TokenAttention(torch.autograd.Function):
    """Forward: the kernel on the views as they lie; no score tensor is kept.  Backward, by the route read in the
    forward (``token_attention_backward_route``): ``"kernel"`` -- the forward ran ``waldo_token_attention_fwd_lse`` and
    saved ``out`` and ``lse`` with the views, and ``waldo_token_attention_bwd`` computes only the wanted gradients in one
    call; ``"framework"`` -- the framework sequence recomputed from the saved views under ``enable_grad`` and
    differentiated.  A forward none of whose inputs needs a gradient runs the plain entry point and allocates no
    ``lse``."""

    @staticmethod
    def forward(ctx, scale, strides, route, q, k, v, k2, v2):
        b, nq, h, d = q.shape
        out = torch.empty(b, nq, h * d, dtype=torch.float32, device=q.device)
        flat = []
        for t, s in zip((q, k, v), strides):
            flat += [t, s[0], s[1]]
        if k2 is not None:
            flat += [k2, strides[3][0], strides[3][1], v2, strides[4][0], strides[4][1]]
        else:
            flat += [None, 0, 0, None, 0, 0]
        shape = (b, h, d, nq, k.shape[1], 0 if k2 is None else k2.shape[1])
        ctx.route = route
        ctx.scale = scale
        ctx.two = k2 is not None
        views = (q, k, v, k2, v2) if ctx.two else (q, k, v)
        if route == "kernel":
            lse = torch.empty(b, h, nq, dtype=torch.float32, device=q.device)
            _lib.launch("waldo_token_attention_fwd_lse", q.device, *flat, out, lse, float(scale), *shape)
            ctx.flat, ctx.shape = [a if type(a) is int else None for a in flat], shape
            ctx.save_for_backward(*views, out, lse)
        else:
            _lib.launch("waldo_token_attention_fwd", q.device, *flat, out, float(scale), *shape)
            ctx.save_for_backward(*views)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        nv = 5 if ctx.two else 3
        need = ctx.needs_input_grad[3:3 + nv]
        if ctx.route == "kernel":
            *views, out, lse = ctx.saved_tensors
            dev = out.device
            grads = [torch.empty(t.shape, dtype=torch.float32, device=dev) if n else None for t, n in zip(views, need)]
            flat = list(ctx.flat)
            flat[0:nv * 3:3] = views
            delta = torch.empty_like(lse)
            # the kernel reads grad_out as dense rows in 16-byte pieces; autograd also hands over strided gradients and
            # contiguous views off that boundary (the gradient of a ``cat``): one copy then, an ordinary op in a graph
            if not grad_out.is_contiguous() or grad_out.data_ptr() % 16:
                grad_out = grad_out.clone(memory_format=torch.contiguous_format)
            _lib.launch("waldo_token_attention_bwd", dev, *flat, out, grad_out, lse, delta, *grads,
                        *([None] * (5 - nv)), float(ctx.scale), *ctx.shape)
            return (None, None, None, *grads, *([None] * (5 - nv)))
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(n) for t, n in zip(ctx.saved_tensors, need)]
            out = token_attention_framework(*leaves, scale=ctx.scale)
            wanted = [t for t, n in zip(leaves, need) if n]
            grads = iter(torch.autograd.grad(out, wanted, grad_out)) if wanted else iter(())
        res = [next(grads) if n else None for n in need]
        return (None, None, None, *res, *([None] * (5 - len(res))))


class _TokenAttention16(torch.autograd.Function):
    """``_TokenAttention`` on bf16 / fp16 operands, ``out`` of the operands' type, by the route read in the forward
    (``token_attention_16bit_backward_route``; ``token_attention_backward_route`` does not reach here).
    ``"framework"``: the forward is ``waldo_token_attention_fwd_dt`` on the views as they lie and the backward the
    ``"framework"`` one of ``_TokenAttention`` -- ``token_attention_framework`` recomputed from the saved views and
    differentiated.  ``"kernel"``: the forward is ``waldo_token_attention_fwd_lse_dt`` and saves ``out`` and the fp32
    ``lse`` with the views; the backward allocates ``delta`` and the wanted gradients and makes one
    ``waldo_token_attention_bwd_dt`` call."""

    @staticmethod
    def forward(ctx, scale, strides, code, route, q, k, v, k2, v2):
        b, nq, h, d = q.shape
        out = torch.empty(b, nq, h * d, dtype=q.dtype, device=q.device)
        flat = []
        for t, s in zip((q, k, v), strides):
            flat += [t, s[0], s[1]]
        if k2 is not None:
            flat += [k2, strides[3][0], strides[3][1], v2, strides[4][0], strides[4][1]]
        else:
            flat += [None, 0, 0, None, 0, 0]
        shape = (b, h, d, nq, k.shape[1], 0 if k2 is None else k2.shape[1], code)
        ctx.route, ctx.scale, ctx.two = route, scale, k2 is not None
        views = (q, k, v, k2, v2) if ctx.two else (q, k, v)
        if route == "kernel":
            lse = torch.empty(b, h, nq, dtype=torch.float32, device=q.device)
            _lib.launch("waldo_token_attention_fwd_lse_dt", q.device, *flat, out, lse, float(scale), *shape)
            ctx.flat, ctx.shape = [a if type(a) is int else None for a in flat], shape
            ctx.save_for_backward(*views, out, lse)
        else:
            _lib.launch("waldo_token_attention_fwd_dt", q.device, *flat, out, float(scale), *shape)
            ctx.save_for_backward(*views)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        nv = 5 if ctx.two else 3
        need = ctx.needs_input_grad[4:4 + nv]
        if ctx.route != "kernel":
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(n) for t, n in zip(ctx.saved_tensors, need)]
                out = token_attention_framework(*leaves, scale=ctx.scale)
                wanted = [t for t, n in zip(leaves, need) if n]
                grads = iter(torch.autograd.grad(out, wanted, grad_out)) if wanted else iter(())
            res = [next(grads) if n else None for n in need]
            return (None, None, None, None, *res, *([None] * (5 - len(res))))
        *views, out, lse = ctx.saved_tensors
        dev = out.device
        grads = [torch.empty(t.shape, dtype=out.dtype, device=dev) if n else None for t, n in zip(views, need)]
        flat = list(ctx.flat)
        flat[0:nv * 3:3] = views
        delta = torch.empty_like(lse)
        # dense rows of the operands' type in 16-byte pieces (see _TokenAttention.backward): one copy otherwise
        if grad_out.dtype != out.dtype:
            grad_out = grad_out.to(out.dtype, memory_format=torch.contiguous_format)
        if not grad_out.is_contiguous() or grad_out.data_ptr() % 16:
            grad_out = grad_out.clone(memory_format=torch.contiguous_format)
        _lib.launch("waldo_token_attention_bwd_dt", dev, *flat, out, grad_out, lse, delta, *grads,
                    *([None] * (5 - nv)), float(ctx.scale), *ctx.shape)
        return (None, None, None, None, *grads, *([None] * (5 - nv)))


def token_attention(q, k, v, k2=None, v2=None, scale=None):
    """``softmax(scale q k^T) v`` per head over the keys of (k, v) followed by those of (k2, v2): q (B, Nq, H, D) and
    k / v (B, Nk, H, D), k2 / v2 (B, Nk2, H, D) or None -> (B, Nq, H D), the layout the output projection takes.
    ``scale``: ``D ** -0.5`` when None.  The operands are VIEWS and are not copied: the slices of a packed ``qkv`` or
    ``kv`` projection as they lie (``qkv.view(B, N, 3, H, D)[:, :, i]``).

    fp32 tensors on the GPU with D in ``token_attention_limits()["head_dims"]``, a unit inner stride, heads D apart
    and rows on 16-byte boundaries run ``waldo_token_attention_fwd`` (include/waldo_hip.h "Token attention"): no score
    tensor, no atomics -- the same bits from run to run in either deterministic mode.  Its backward takes the route
    set by ``token_attention_backward_route``: ``"kernel"`` is ``waldo_token_attention_bwd`` (the forward then also
    stores its row statistics, ``waldo_token_attention_fwd_lse``; no score tensor, no atomics, only the wanted
    gradients), ``"framework"`` recomputes ``token_attention_framework`` from the saved views and differentiates that.
    bf16 / fp16 tensors on the GPU run ``waldo_token_attention_fwd_dt`` -- both products on the 16-bit matrix
    instruction with fp32 accumulation, the softmax in fp32, ``out`` of the operands' type -- ONLY under
    ``token_attention_16bit_route("kernel")``, then also while autocast is enabled; their strides are multiples of 8
    elements.  Such a call differentiates by the ``"framework"`` route whatever ``token_attention_backward_route``
    says; its own switch, ``token_attention_16bit_backward_route("kernel")``, gives it ``waldo_token_attention_bwd_dt``
    (the forward then is ``waldo_token_attention_fwd_lse_dt``; gradients of the operands' type).
    Everything else -- CPU tensors, another D, another dtype (16-bit inputs under the default 16-bit route, autocast),
    another layout -- IS ``token_attention_framework`` end to end."""
    _token_attention_check(q, k, v, k2, v2)
    scale = q.shape[3] ** -0.5 if scale is None else float(scale)
    strides = _token_attention_served(q, k, v, k2, v2)
    if strides is None:
        strides = _token_attention_served_16bit(q, k, v, k2, v2)
        if strides is not None:
            # (as below: the route travels with the node, and a call that records no node needs no row statistics)
            route = _token_attention_16bit_backward_route
            if route == "kernel" and not (torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                                                          for t in (q, k, v, k2, v2))):
                route = "framework"
            return _TokenAttention16.apply(scale, strides, _DTYPE_CODE[q.dtype], route, q, k, v, k2, v2)
        return token_attention_framework(q, k, v, k2, v2, scale)
    # the route travels with the node; a call that records no node (no gradient wanted) needs no row statistics
    route = _token_attention_backward_route
    if route == "kernel" and not (torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                                                  for t in (q, k, v, k2, v2))):
        route = "framework"
    return _TokenAttention.apply(scale, strides, route, q, k, v, k2, v2)


# --------------------------------------------------------------------------------------
# token attention over clips: per-clip segments of packed rows (the future layer predictor's blocks under ctx_mask)
# --------------------------------------------------------------------------------------
def clip_offsets(ctx_mask, tokens_per_frame):
    """The offset table of a boolean (B, T) frame mask whose selected frames carry ``tokens_per_frame`` packed rows each:
    int32 (B + 1,), clip b's rows are ``[off[b], off[b + 1])``.  A ``cumsum`` on the mask's device; no host read."""
    if ctx_mask.dim() != 2:
        raise ValueError(f"clip_offsets: ctx_mask must be (B, T), got {tuple(ctx_mask.shape)}")
    off = torch.zeros(ctx_mask.shape[0] + 1, dtype=torch.int32, device=ctx_mask.device)
    off[1:] = torch.cumsum(ctx_mask.sum(dim=1, dtype=torch.int32) * int(tokens_per_frame), dim=0)
    return off


def _token_attention_clips_check(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len):
    if q.dim() != 3:
        raise ValueError(f"token_attention_clips: q must be (Rq, H, D), got {tuple(q.shape)}")
    _, h, d = q.shape
    if k.dim() != 3 or tuple(k.shape[1:]) != (h, d) or v.shape != k.shape:
        raise ValueError(f"token_attention_clips: k and v must be (Rk, {h}, {d}), got {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    for name, off in (("q_offsets", q_offsets), ("k_offsets", k_offsets)):
        if off.dim() != 1 or off.numel() < 1 or off.dtype != torch.int32 or off.device != q.device:
            raise ValueError(f"token_attention_clips: {name} must be int32 (B + 1,) on {q.device}, got {off.dtype} "
                             f"{tuple(off.shape)} on {off.device}")
    if q_offsets.shape != k_offsets.shape:
        raise ValueError(f"token_attention_clips: q_offsets and k_offsets must have B + 1 entries each, got "
                         f"{tuple(q_offsets.shape)}, {tuple(k_offsets.shape)}")
    if int(max_q_len) < 0 or int(max_k_len) < 0:
        raise ValueError(f"token_attention_clips: max_q_len and max_k_len must be >= 0, got {max_q_len}, {max_k_len}")


def _clip_of_rows(offsets, rows):
    """The clip of each of ``rows`` packed rows: the number of clip ends at or before the row (no host read)."""
    return torch.bucketize(torch.arange(rows, device=offsets.device, dtype=torch.int32), offsets[1:], right=True)


def token_attention_clips_framework(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len, scale=None):
    """``token_attention_clips`` in framework ops: the scores of all Rq x Rk rows under a block mask (the clip of the
    query is not the clip of the key -> -inf), softmax, the values.  The clip of a row comes from ``bucketize`` on the
    offsets, so nothing is read on the host.  A query row whose clip has no key is a softmax over -inf alone: NaN, as
    in the reference.  The CPU route of ``token_attention_clips``, the ``fused = False`` route of the future layer
    predictor's blocks, the fallback for operands the kernel does not serve and what its ``"framework"`` backward
    route differentiates.  ``max_q_len`` / ``max_k_len`` only size the kernel's grid and are not used here."""
    _token_attention_clips_check(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len)
    rq, h, d = q.shape
    scale = d ** -0.5 if scale is None else scale
    attn = (q.permute(1, 0, 2) @ k.permute(1, 2, 0)) * scale
    other = _clip_of_rows(q_offsets, rq)[:, None] != _clip_of_rows(k_offsets, k.shape[0])[None, :]
    attn = attn.masked_fill(other, float("-inf")).softmax(dim=-1)
    return (attn @ v.permute(1, 0, 2)).transpose(0, 1).reshape(rq, h * d)


def _packed_view_stride(t):
    """The token stride of a (R, H, D) view whose (row, head) rows are D consecutive floats D apart and start on 16-byte
    boundaries -- what ``waldo_token_attention_clips_fwd`` reads in place -- else None."""
    r, h, d = t.shape
    if (d > 1 and t.stride(2) != 1) or (h > 1 and t.stride(1) != d) or t.data_ptr() % 16:
        return None
    sn = t.stride(0) if r > 1 else 0
    return None if sn % 4 or sn < 0 else sn


def _token_attention_clips_served(q, k, v, q_offsets, k_offsets):
    """The token strides of the operands if the kernel serves them as they lie, else None."""
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == q.device for t in (q, k, v)):
        return None
    if q.shape[2] not in token_attention_limits()["head_dims"] or q.numel() == 0 or k.numel() == 0:
        return None
    if not (q_offsets.is_contiguous() and k_offsets.is_contiguous()) or torch.is_autocast_enabled("cuda"):
        return None
    strides = [_packed_view_stride(t) for t in (q, k, v)]
    return None if any(s is None for s in strides) else strides


def _token_attention_clips_served_16bit(q, k, v, q_offsets, k_offsets):
    """``_token_attention_served_16bit`` for the packed operands of ``token_attention_clips``: their token strides, or
    None."""
    if _token_attention_16bit_route != "kernel" or not _same_16bit_on_gpu((q, k, v)):
        return None
    if q.shape[2] not in token_attention_16bit_limits()["head_dims"] or q.numel() == 0 or k.numel() == 0:
        return None
    if not (q_offsets.is_contiguous() and k_offsets.is_contiguous()):
        return None
    strides = []
    for t in (q, k, v):
        r, h, d = t.shape
        sn = t.stride(0) if r > 1 else 0
        if (d > 1 and t.stride(2) != 1) or (h > 1 and t.stride(1) != d) or t.data_ptr() % 16 or sn % 8 or sn < 0:
            return None
        strides.append(sn)
    return strides


class _TokenAttentionClips(torch.autograd.Function):
    """``_TokenAttention`` for per-clip segments: the kernel on the packed views as they lie; the backward by the route
    read in the forward -- ``"kernel"``: ``waldo_token_attention_clips_bwd`` from the saved ``out`` and ``lse``;
    ``"framework"``: ``token_attention_clips_framework`` recomputed from the saved views and differentiated."""

    @staticmethod
    def forward(ctx, scale, strides, route, bounds, q, k, v, q_offsets, k_offsets):
        rq, h, d = q.shape
        out = torch.empty(rq, h * d, dtype=torch.float32, device=q.device)
        flat = [q, strides[0], k, strides[1], v, strides[2], q_offsets, k_offsets]
        shape = (q_offsets.numel() - 1, h, d, rq, k.shape[0], int(bounds[0]), int(bounds[1]))
        ctx.route, ctx.scale, ctx.strides, ctx.shape = route, scale, strides, shape
        if route == "kernel":
            lse = torch.empty(h, rq, dtype=torch.float32, device=q.device)
            _lib.launch("waldo_token_attention_clips_fwd_lse", q.device, *flat, out, lse, float(scale), *shape)
            ctx.save_for_backward(q, k, v, q_offsets, k_offsets, out, lse)
        else:
            _lib.launch("waldo_token_attention_clips_fwd", q.device, *flat, out, float(scale), *shape)
            ctx.save_for_backward(q, k, v, q_offsets, k_offsets)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad[4:7]
        if ctx.route == "kernel":
            q, k, v, q_offsets, k_offsets, out, lse = ctx.saved_tensors
            # (empty: the kernel overwrites every row that belongs to a clip, and the tables of a plan cover all rows)
            grads = [torch.empty(t.shape, dtype=torch.float32, device=out.device) if n else None
                     for t, n in zip((q, k, v), need)]
            delta = torch.empty_like(lse)
            if not grad_out.is_contiguous() or grad_out.data_ptr() % 16:  # (see _TokenAttention.backward)
                grad_out = grad_out.clone(memory_format=torch.contiguous_format)
            s = ctx.strides
            _lib.launch("waldo_token_attention_clips_bwd", out.device, q, s[0], k, s[1], v, s[2], q_offsets, k_offsets,
                        out, grad_out, lse, delta, *grads, float(ctx.scale), *ctx.shape)
            return (None, None, None, None, *grads, None, None)
        q, k, v, q_offsets, k_offsets = ctx.saved_tensors
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(n) for t, n in zip((q, k, v), need)]
            out = token_attention_clips_framework(*leaves, q_offsets, k_offsets, ctx.shape[5], ctx.shape[6],
                                                  scale=ctx.scale)
            wanted = [t for t, n in zip(leaves, need) if n]
            grads = iter(torch.autograd.grad(out, wanted, grad_out)) if wanted else iter(())
        return (None, None, None, None, *[next(grads) if n else None for n in need], None, None)


class _TokenAttentionClips16(torch.autograd.Function):
    """``_TokenAttentionClips`` on bf16 / fp16 operands: ``waldo_token_attention_clips_fwd_dt`` forward, and always the
    ``"framework"`` backward of ``_TokenAttentionClips`` (no 16-bit backward kernel)."""

    @staticmethod
    def forward(ctx, scale, strides, code, bounds, q, k, v, q_offsets, k_offsets):
        rq, h, d = q.shape
        out = torch.empty(rq, h * d, dtype=q.dtype, device=q.device)
        shape = (q_offsets.numel() - 1, h, d, rq, k.shape[0], int(bounds[0]), int(bounds[1]))
        ctx.route, ctx.scale, ctx.strides, ctx.shape = "framework", scale, strides, shape
        _lib.launch("waldo_token_attention_clips_fwd_dt", q.device, q, strides[0], k, strides[1], v, strides[2],
                    q_offsets, k_offsets, out, float(scale), *shape, code)
        ctx.save_for_backward(q, k, v, q_offsets, k_offsets)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return _TokenAttentionClips.backward(ctx, grad_out)


def token_attention_clips(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len, scale=None):
    """``softmax(scale q k^T) v`` per head within each clip of PACKED rows: q (Rq, H, D) and k / v (Rk, H, D) hold the
    rows of all clips one after the other, clip b's queries are the rows ``[q_offsets[b], q_offsets[b + 1])`` and its
    keys the rows ``[k_offsets[b], k_offsets[b + 1])`` -> (Rq, H D).  The offsets are int32 (B + 1,) tensors on the
    operands' device (``clip_offsets``) and must cover the rows: a row that belongs to no clip is not written.
    ``max_q_len`` / ``max_k_len`` are host integers no clip's length exceeds (the kernel's grid; a clip longer than its
    bound is served up to the bound only).  ``scale``: ``D ** -0.5`` when None.  The operands are VIEWS and are not
    copied: the slices of a packed ``qkv`` / ``kv`` projection as they lie (``qkv.view(R, 3, H, D)[:, i]``).

    This is the reference's attention under ``ctx_mask`` (models/modules/transform.py: ``from_ctx``, a dense -inf mask
    over all T N keys, ``to_ctx``) without the dense tensors and without their host reads: nothing here reads the
    offsets on the host, so a call can be captured in a graph.  A clip with queries and no keys gives NaN in its rows.

    fp32 tensors on the GPU that ``waldo_token_attention_clips_fwd`` serves (as ``token_attention``: D in
    ``token_attention_limits()["head_dims"]``, unit inner stride, heads D apart, rows on 16-byte boundaries, Rk > 0)
    run the kernel, with the backward set by ``token_attention_backward_route``; bf16 / fp16 tensors run
    ``waldo_token_attention_clips_fwd_dt`` under ``token_attention_16bit_route("kernel")`` (as ``token_attention``:
    forward only, the ``"framework"`` backward); everything else IS ``token_attention_clips_framework``."""
    _token_attention_clips_check(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len)
    scale = q.shape[2] ** -0.5 if scale is None else float(scale)
    strides = _token_attention_clips_served(q, k, v, q_offsets, k_offsets)
    if strides is None:
        strides = _token_attention_clips_served_16bit(q, k, v, q_offsets, k_offsets)
        if strides is not None:
            return _TokenAttentionClips16.apply(scale, strides, _DTYPE_CODE[q.dtype], (int(max_q_len), int(max_k_len)),
                                                q, k, v, q_offsets, k_offsets)
        return token_attention_clips_framework(q, k, v, q_offsets, k_offsets, max_q_len, max_k_len, scale)
    route = _token_attention_backward_route
    if route == "kernel" and not (torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))):
        route = "framework"
    return _TokenAttentionClips.apply(scale, strides, route, (int(max_q_len), int(max_k_len)), q, k, v, q_offsets,
                                      k_offsets)


def lpips_level_framework(f0, f1, w, eps=1e-10):
    """``lpips_level`` in framework ops, as the ``lpips`` package spells it: ``normalize_tensor`` (eps added after the
    square root), the squared difference, the bias-free 1 x 1 lin convolution, ``spatial_average``.  Any device and
    floating dtype; differentiable in every operand."""
    u0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + eps)
    u1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + eps)
    d = torch.nn.functional.conv2d((u0 - u1) ** 2, w.reshape(1, -1, 1, 1))
    return d.mean([2, 3]).reshape(-1)


def _lpips_level_call(f0, f1, w, eps, want_saved):
    """One forward call on dense operands (fp32, or 16-bit maps with an fp32 ``w``): (out (N,), saved or None)."""
    n, c, h, wd = f0.shape
    p, dev = h * wd, f0.device
    nbytes = _lib.query("waldo_lpips_level_workspace_bytes", n, c, p)
    if nbytes <= 0:
        raise ValueError(f"lpips_level: unsupported shape {tuple(f0.shape)} (C H W at most 2^31 - 1)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    saved = None
    if want_saved:
        saved = torch.empty(_lib.query("waldo_lpips_level_saved_bytes", n, c, p) // 4, dtype=torch.float32, device=dev)
    name, codes = _dt_entry("waldo_lpips_level_fwd", f0.dtype)
    _lib.launch(name, dev, f0, f1, w, out, saved, ws, nbytes, n, c, p, float(eps), *codes)
    return out, saved


class _LpipsLevel(torch.autograd.Function):
    """``waldo_lpips_level_fwd`` (``_fwd_dt`` for 16-bit maps) with the per-pixel values its backward needs kept only when
    ``f0`` asks for a gradient; ``grad_f1`` is the same pair of calls with the operands exchanged (the distance is
    symmetric), its forward run in the backward: the loss differentiates the prediction alone.  ``out`` and ``grad_out``
    are fp32; the gradients have the maps' type."""

    @staticmethod
    def forward(ctx, eps, f0, f1, w):
        f0, f1, w = f0.contiguous(), f1.contiguous(), w.contiguous()
        out, saved = _lpips_level_call(f0, f1, w, eps, ctx.needs_input_grad[1])
        ctx.eps = eps
        ctx.save_for_backward(f0, f1, w, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        f0, f1, w, saved = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        n, c, h, wd = f0.shape
        name, codes = _dt_entry("waldo_lpips_level_bwd", f0.dtype)
        grads = [None, None]
        for i, (a, b) in enumerate(((f0, f1), (f1, f0))):
            if not ctx.needs_input_grad[1 + i]:
                continue
            if i == 1:
                _, saved = _lpips_level_call(a, b, w, ctx.eps, True)
            grads[i] = torch.empty_like(a)
            _lib.launch(name, a.device, a, b, w, saved, grad_out, grads[i], n, c, h * wd, *codes)
        return (None, grads[0], grads[1], None)


def _lpips_level_mixed(f0, w):
    return f0.dtype in (torch.bfloat16, torch.float16) and w.dtype == torch.float32


def _lpips_level_check(f0, f1, w):
    for name, t in (("f0", f0), ("f1", f1)):
        if not torch.is_tensor(t) or t.ndim != 4 or not t.is_floating_point():
            raise ValueError(f"lpips_level: {name} must be a floating (N, C, H, W) tensor, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    if f0.shape != f1.shape or f0.dtype != f1.dtype or f0.device != f1.device:
        raise ValueError(f"lpips_level: f0 and f1 disagree: {f0.dtype} {tuple(f0.shape)} on {f0.device} and {f1.dtype} "
                         f"{tuple(f1.shape)} on {f1.device}")
    if f0.numel() == 0:
        raise ValueError(f"lpips_level: the operands {tuple(f0.shape)} are empty")
    mixed = torch.is_tensor(w) and _lpips_level_mixed(f0, w)  # 16-bit maps with an fp32 w: what autocast produces
    if not torch.is_tensor(w) or w.numel() != f0.shape[1] or not (w.dtype == f0.dtype or mixed) or w.device != f0.device:
        raise ValueError(f"lpips_level: w must hold C = {f0.shape[1]} {f0.dtype} weights on {f0.device}"
                         f"{' (or float32 ones)' if f0.dtype in (torch.bfloat16, torch.float16) else ''}, got "
                         f"{getattr(w, 'dtype', type(w).__name__)} {tuple(getattr(w, 'shape', ()))}"
                         + (f" on {w.device}" if torch.is_tensor(w) else ""))


def lpips_level(f0, f1, w, eps=1e-10):
    """The tail of LPIPS at one feature level: ``f0``, ``f1`` (N, C, H, W) feature maps, ``w`` the lin layer's C weights
    (any shape of C elements: ``lin.model[1].weight`` as it is) -> (N,)::

        u = f / (sqrt(sum_c f^2) + eps);   out[n] = mean over pixels of sum_c w[c] (u0 - u1)^2

    The kernels (include/waldo_hip.h "LPIPS level distance"): the two maps are read, one float per image is written; no
    atomics -- the same bits from run to run; ``f1 == f0`` gives exact zeros, value and gradient; a pixel of ``f0`` that
    is zero on every channel gets an exact 0 gradient (the framework chain: NaN from the square root's backward, which
    the ReLU behind every LPIPS tap turns into 0 as well).  Operands that are not contiguous are made so.  The routes:

    ===================================================  ===========================================================
    fp32 maps and ``w`` on the GPU, ``w`` needs no grad  ``waldo_lpips_level_fwd`` / ``_bwd``
    bf16 / fp16 maps with an FP32 ``w`` (what autocast   ``waldo_lpips_level_fwd_dt`` / ``_bwd_dt``: fp32 arithmetic on
    hands over) on the GPU, ``w`` needs no grad          the widened maps; ``out`` is fp32, the gradients have the
                                                         maps' type, rounded once (fp16: scale the loss)
    the same maps on the CPU, or ``w.requires_grad``     ``lpips_level_framework`` on the maps widened to fp32:
                                                         ``out`` fp32, gradients of the maps' type
    everything else (CPU, fp64, ``w.requires_grad``,     IS ``lpips_level_framework`` in the operands' type
    16-bit maps with a ``w`` of the SAME 16-bit type)
    ===================================================  ==========================================================="""
    _lpips_level_check(f0, f1, w)
    if _lpips_level_mixed(f0, w):
        if f0.is_cuda and not w.requires_grad:
            return _LpipsLevel.apply(float(eps), f0, f1, w.detach().reshape(-1))
        return lpips_level_framework(f0.float(), f1.float(), w, eps)
    if f0.is_cuda and f0.dtype == torch.float32 and not w.requires_grad:
        return _LpipsLevel.apply(float(eps), f0, f1, w.detach().reshape(-1))
    return lpips_level_framework(f0, f1, w, eps)
