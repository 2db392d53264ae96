"""Dtype-agnostic restatement, in framework ops, of the lines of the reference that ``waldo_amd.supervision`` replaces --
the yardstick of tests/test_supervision_cpu.py and tests/test_gpu_supervision.py, run in fp32 and in fp64 from the same
inputs (tests/parity.py).  Every function cites the lines it restates and keeps their order of operations.

The blur is written from the DEFINITION of torchvision's ``GaussianBlur(kernel_size, sigma)`` (1-D weights
``exp(-(t / sigma)^2 / 2)`` at ``t = linspace(-(k - 1) / 2, (k - 1) / 2, k)``, normalised; the 2-D kernel their outer
product; reflection padding; depthwise ``conv2d``): torchvision itself is not a dependency of the tests, so the blur is
checked against this restatement and never against torchvision."""
import math

import torch
import torch.nn.functional as F

from waldo_amd.tools.utils import get_grid


def edge_kernels(k, dtype):
    """models/modules/edge.py:15-26: the mean kernel and the two gradient kernels (2, 1, k, k).  The reference's buffers
    are fp32 (its integer tensors divide to fp32): they are built so and only then cast, so that the fp64 evaluation
    filters with the same weights and differs from the fp32 one by the arithmetic alone."""
    mean = torch.ones(1, 1, k, k) / (k ** 2)
    sobel = torch.tensor(list(range(k))) - k // 2
    sobel_x, sobel_y = sobel.view(-1, 1), sobel.view(1, -1)
    sum_xy = sobel_x ** 2 + sobel_y ** 2
    sum_xy[sum_xy == 0] = 1
    sobel_x, sobel_y = sobel_x / sum_xy, sobel_y / sum_xy
    assert sobel_x.dtype == torch.float32
    return mean.to(dtype), torch.stack([sobel_x.unsqueeze(0), sobel_y.unsqueeze(0)], dim=0).to(dtype)


def flow_edges_parts(flow, k=15, eps=1e-6):
    """edge.py:28-40 on (..., C, H, W): (flow_edge, dominant_flow, flow_norm - mean_flow_norm), the last being the
    quantity whose sign decides ``dominant_flow``."""
    lead = flow.shape[:-3]
    x = flow.reshape(-1, *flow.shape[-3:])
    b, c, h, w = x.shape
    mean_k, sobel_k = edge_kernels(k, x.dtype)
    mean_k, sobel_k = mean_k.to(x.device), sobel_k.to(x.device)
    pad = F.pad(x.reshape(b * c, 1, h, w), (k // 2,) * 4, mode="reflect")
    mean_flow = F.conv2d(pad, mean_k)
    mean_flow_norm = (mean_flow.view(b, c, h, w) ** 2).sum(dim=1, keepdim=True)
    flow_norm = (x ** 2).sum(dim=1, keepdim=True)
    dominant = (flow_norm > mean_flow_norm).to(x.dtype)
    edge = F.conv2d(pad, sobel_k)
    edge = ((edge ** 2).sum(dim=1, keepdim=True) + eps).sqrt() / math.sqrt(32)
    edge = 1 - (1 - edge.view(b, c, h, w)).prod(dim=1, keepdim=True)
    one = (*lead, 1, h, w)
    return edge.view(one), dominant.view(one), (flow_norm - mean_flow_norm).view(one)


def flow_edges(flow, k=15, eps=1e-6):
    return flow_edges_parts(flow, k, eps)[:2]


def gaussian_weights(k, sigma, dtype):
    """torchvision's 1-D kernel: ``pdf = exp(-0.5 (x / sigma)^2)`` at ``x = linspace(-half, half, k)``, ``pdf / sum``."""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=dtype)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(x, sigma, k=23):
    """models/synthesizer.py:1114-1118 through the definition in the module docstring."""
    w1 = gaussian_weights(k, sigma, x.dtype).to(x.device)
    img = x.reshape(-1, *x.shape[-3:])
    c = img.shape[1]
    kernel = (w1[:, None] * w1[None, :]).expand(c, 1, k, k)
    out = F.conv2d(F.pad(img, (k // 2,) * 4, mode="reflect"), kernel, groups=c)
    return out.view_as(x)


def moving_object_target(real_flow, real_lyt, fg_idx, bg_idx, other_idx, *, flow_thresh, mov_obj_thresh, blur_sigma,
                         edge_size, reg_bg_mul=0.25, use_fg=False, use_nobg=False, use_nobg_edge=False, nobg_edge_mul=0.0,
                         use_flow_nobg=False, use_dominant_flow_other=False):
    """models/synthesizer.py:907-942 with ``blur_alpha`` off, on (B, T, C, H, W).  Returns a dict: the fields of
    ``supervision.MovingObjectTarget`` plus the deciding quantities ``edge_raw`` (before its threshold), ``delta_flow``
    and ``dominant_margin``."""
    flow_edge_raw, dominant_flow, dominant_margin = flow_edges_parts(real_flow, edge_size)
    flow_edge = (flow_edge_raw > flow_thresh).to(real_flow.dtype)
    fg_prop = (real_lyt[:, :, list(fg_idx)] / 10 + 1 / 2).sum(dim=2, keepdim=True)
    nofg_prop = 1 - fg_prop
    bg_prop = (real_lyt[:, :, list(bg_idx)] / 10 + 1 / 2).sum(dim=2, keepdim=True)
    nobg_prop = 1 - bg_prop
    nofg_flow = gaussian_blur(torch.cat([nofg_prop, nofg_prop * real_flow], dim=2), blur_sigma)
    sum_nofg_flow = nofg_flow[:, :, :1] + (nofg_flow[:, :, :1] == 0).to(real_flow.dtype)
    mean_bg_flow = nofg_flow[:, :, 1:] / sum_nofg_flow
    delta_flow = fg_prop * (real_flow - mean_bg_flow).abs().sum(dim=2, keepdim=True)
    mov_obj_mask = delta_flow > mov_obj_thresh
    if use_dominant_flow_other:
        other_prop = (real_lyt[:, :, list(other_idx)] / 10 + 1 / 2).sum(dim=2, keepdim=True)
        mov_obj_mask = torch.max(mov_obj_mask.to(real_flow.dtype), other_prop * dominant_flow * flow_edge)
    if use_flow_nobg:
        flow_mask = (flow_edge > 0.1) & (nobg_prop > 0)
        mov_obj_mask = mov_obj_mask | flow_mask
    mov_obj_mask = mov_obj_mask.to(real_flow.dtype)
    mov_obj = mov_obj_mask * 2 - 1
    mov_obj[mov_obj < 0] *= reg_bg_mul
    if use_fg:
        mov_obj[(mov_obj < 0) & (fg_prop > 0)] = 0
    if use_nobg:
        mov_obj[(mov_obj < 0) & (nobg_prop > 0)] = 0
    if use_nobg_edge:
        mov_obj[(mov_obj < 0) & (nobg_prop > 0) & (flow_edge > 0.1)] = nobg_edge_mul
    return dict(mov_obj_mask=mov_obj_mask, mov_obj=mov_obj, fg_prop=fg_prop, mean_bg_flow=mean_bg_flow,
                flow_edge=flow_edge, dominant_flow=dominant_flow, edge_raw=flow_edge_raw, delta_flow=delta_flow,
                dominant_margin=dominant_margin, nobg_prop=nobg_prop)


def cell_distance(obj_pose, obj_shape, mov_obj_mask, fg_mask, eps=0.0):
    """models/synthesizer.py:965-979, with its (B, T, No, cells, H, W) tensor: (cell_dis, center_dis)."""
    h, w = mov_obj_mask.shape[-2:]
    grid = get_grid(h, w).to(obj_pose)
    no = obj_pose.shape[2]
    obj_grid = obj_pose.view(*obj_pose.shape[:3], *obj_shape, 2)
    obj_cell = (obj_grid[:, :, :, 1:, 1:] + obj_grid[:, :, :, 1:, :-1] + obj_grid[:, :, :, :-1, 1:]
                + obj_grid[:, :, :, :-1, :-1]) / 4
    obj_center = obj_grid.view(*obj_pose.shape[:3], -1, 2).mean(dim=3)
    obj_cell_dis = (grid ** 2).sum(dim=-1).view(1, -1) + (obj_cell ** 2).sum(dim=-1).view(-1, 1) \
        - 2 * obj_cell.reshape(-1, 2) @ grid.view(-1, 2).t()
    obj_cell_dis = obj_cell_dis.view(*obj_grid.shape[:2], no, -1, *grid.shape[1:3]).sum(dim=3)
    obj_center_dis = (grid ** 2).sum(dim=-1).view(1, -1) + (obj_center ** 2).sum(dim=-1).view(-1, 1) \
        - 2 * obj_center.reshape(-1, 2) @ grid.view(-1, 2).t()
    obj_center_dis = obj_center_dis.view(*obj_grid.shape[:2], no, *grid.shape[1:3])
    cell_dis = ((mov_obj_mask + eps) * (1 - fg_mask) * obj_cell_dis).min(dim=2)[0].mean()
    center_dis = (mov_obj_mask * obj_center_dis).min(dim=2)[0].mean()
    return cell_dis, center_dis


def recipe_terms(alpha_flt, rec_flow, real_flow, real_lyt, obj_pose, obj_shape, target, cell_dis_eps=0.0):
    """The recipe's four terms (scripts/cityscapes/train_lvd.sh:15) with ``swap_flt``: synthesizer.py:888-899
    (ent_flt_edge), :931 and :951 (reg_mov), :977 (cell_dis), :989 (l1_flow).  ``target``: ``moving_object_target``'s
    dict."""
    entropy_flt = (alpha_flt + 1) / 2
    entropy_flt = F.normalize(entropy_flt + 1e-6, p=1, dim=2)
    entropy_flt = -torch.sum(torch.mul(entropy_flt, torch.log(entropy_flt + 1e-6)), dim=2, keepdim=True) / 0.37
    lyt_edge_mask = (gaussian_blur(real_lyt / 10 + 1 / 2, 2, 3).max(dim=2, keepdim=True)[0] > 0.999).to(alpha_flt.dtype)
    fg_mask = ((alpha_flt[:, :, 1:] + 1) / 2).sum(dim=2, keepdim=True)
    found_obj = -fg_mask
    return {"cell_dis": cell_distance(obj_pose, obj_shape, target["mov_obj_mask"], fg_mask, cell_dis_eps)[0],
            "reg_mov": (target["mov_obj"] * found_obj).mean(),
            "ent_flt_edge": (entropy_flt * lyt_edge_mask).mean(),
            "l1_flow": (real_flow[:, 1:] - rec_flow).abs().mean()}
