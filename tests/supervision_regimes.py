"""Operands for waldo_amd.supervision at the shapes where its kernels change workgroup: more than one chunk of 2048
pixels for ``cell_distance`` (csrc/supervision.hip: kCellChunk), a second row of the blur's 32 x 64 tiles, a second
row and column of the edges' 16 x 64 tiles -- and at their limits: 31 objects, more than 256 partials, a blur of 31
taps, 32 layout channels.  The builders are seeded; the restatement's results (tests/supervision_ref.py, fp32 and fp64)
are computed once per case and shared by tests/test_gpu_supervision.py, tests/test_supervision_regimes_cpu.py and
tests/test_supervision_sensitivity_cpu.py: do not write to them.  Pure torch on the CPU."""
import functools
import hashlib

import torch

import supervision_ref as R

CELL_CHUNK = 2048                                    # csrc/supervision.hip: kCellChunk = kCellPx * kBlock
FG, BG, OTHER, NL = [0, 3], [1, 2], [4], 6           # (channel 5 is in no list)
THRESH = dict(flow_thresh=0.02, mov_obj_thresh=0.005, blur_sigma=2.0, edge_size=7)
RECIPE_OPTS = dict(use_fg=True, use_dominant_flow_other=True)
ALL_OPTS = dict(use_fg=True, use_nobg=True, use_nobg_edge=True, nobg_edge_mul=-0.5, use_flow_nobg=True)

# (B, T, No, obj_shape, H, W)
CELL_CASES = [(2, 3, 5, (4, 4), 33, 70),     # 2310 px: two chunks, the second of 262 px -- one round of lanes plus six
              (2, 3, 31, (4, 4), 33, 70),    # the object limit: 93 moment words, 93 x 4 reduction slots
              (2, 3, 16, (4, 4), 48, 128),   # exactly three chunks, the recipe's No
              (5, 26, 3, (2, 3), 33, 70)]    # F = 130: 260 partials (> 256), 1170 threads of the moments gradient
BLUR_SHAPES = [(40, 72), (33, 65), (65, 40), (16, 70)]
BLUR_CASES = [(h, w, k, sigma) for h, w in BLUR_SHAPES for k in (3, 23, 31) if min(h, w) > k // 2 for sigma in (2.0, 5.0)]
EDGE_CASES = [(h, w, k) for h, w in ((33, 130), (17, 65)) for k in (3, 15)]
TARGET_CASES = [(h, w, e) for h, w in ((40, 72), (37, 70)) for e in (15, 7)]


def target_inputs(h=24, w=40, nl=NL, seed=7):
    """2 x 3 frames at h x w.  Layouts: one-hot +-5 in 4 x 4 blocks, cropped; frame (0, 1) all foreground (class 0: the
    blurred weight is exactly 0); frame (1, 2) soft.  Flow: smooth, plus a rectangle from about (h / 4, w / 4) to
    (0.7 h, 0.65 w) that moves on its own, plus noise of 5e-4."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, nl, (2, 3, -(-h // 4), -(-w // 4)), generator=g)
    cls = cls.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)[:, :, :h, :w].contiguous()
    cls[0, 1] = 0
    lyt = torch.nn.functional.one_hot(cls, nl).permute(0, 1, 4, 2, 3).float() * 10 - 5
    lyt[1, 2] = 10 * torch.softmax(2 * torch.randn(nl, h, w, generator=g), dim=0) - 5
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    flow = torch.stack([0.012 * torch.sin(2 * xs + ys), 0.008 * torch.cos(1.5 * ys - xs)]).expand(2, 3, 2, h, w).clone()
    flow *= torch.linspace(0.6, 1.4, 6).view(2, 3, 1, 1, 1)
    y0, y1, x0, x1 = round(h / 4), round(0.7 * h), round(w / 4), round(0.65 * w)
    flow[:, :, 0, y0:y1, x0:x1] += 0.03
    flow[:, :, 1, y0:y1, x0:x1] -= 0.02
    flow += 5e-4 * torch.randn(flow.shape, generator=g)
    return flow.contiguous(), lyt.contiguous()


# the six channels of ``target_inputs`` among 32: lists that name channels 31, 30 and 0; the other 26 hold -5 (share 0)
WIDE_NL, WIDE_PLACES = 32, (31, 30, 2, 0, 16, 5)
WIDE_FG, WIDE_BG, WIDE_OTHER = [31, 0], [30, 2], [16]


def wide_inputs(h, w):
    """``target_inputs(h, w)`` with its channels 0 .. 5 moved to WIDE_PLACES of a 32-channel layout."""
    flow, lyt = target_inputs(h, w)
    wide = torch.full((2, 3, WIDE_NL, h, w), -5.0)
    wide[:, :, list(WIDE_PLACES)] = lyt
    return flow, wide.contiguous()


def recipe_clip(h, w, nl=20, seed=13):
    """(flow, clip): a 3 + nl channel clip whose channels 3 .. are the layout of ``target_inputs(h, w, nl)``; the layout
    the recipe's lists are run on is the strided slice ``clip[:, :, 3:]``."""
    flow, lyt = target_inputs(h, w, nl=nl, seed=seed)
    clip = torch.randn(2, 3, 3 + nl, h, w, generator=torch.Generator().manual_seed(seed + 1))
    clip[:, :, 3:] = lyt
    return flow, clip


@functools.lru_cache(maxsize=None)
def target_refs(h=24, w=40, edge_size=THRESH["edge_size"], layout="six"):
    """(flow, lyt, lists, thresh, refs): the inputs and ``refs(**opts)`` -> the restatement's targets (fp32, fp64),
    each computed once per option set."""
    flow, lyt = wide_inputs(h, w) if layout == "wide" else target_inputs(h, w)
    lists = (WIDE_FG, WIDE_BG, WIDE_OTHER) if layout == "wide" else (FG, BG, OTHER)
    thresh = dict(THRESH, edge_size=edge_size)
    cache = {}

    def refs(**opts):
        key = tuple(sorted(opts.items()))
        if key not in cache:
            cache[key] = (R.moving_object_target(flow, lyt, *lists, **thresh, **opts),
                          R.moving_object_target(flow.double(), lyt.double(), *lists, **thresh, **opts))
        return cache[key]

    return flow, lyt, lists, thresh, refs


def cell_inputs(b, t, no, obj_shape, h, w, seed):
    """pose = 0.6 randn, fg = 1.2 rand (some weights 1 - fg are negative), mask = (rand < 0.4)."""
    g = torch.Generator().manual_seed(seed)
    pose = 0.6 * torch.randn(b, t, no, obj_shape[0] * obj_shape[1], 2, generator=g)
    fg = 1.2 * torch.rand(b, t, 1, h, w, generator=g)
    mask = (torch.rand(b, t, 1, h, w, generator=g) < 0.4).float()
    return pose, fg, mask


def cell_seed(case):
    return 100 + CELL_CASES.index(case)


def ref_cell(pose, fg, m, obj_shape, eps, dtype):
    """(cell_dis, center_dis, grad pose of cell_dis, grad fg_mask of cell_dis, grad pose of center_dis)."""
    p, f = (x.detach().to(dtype, copy=True).requires_grad_() for x in (pose, fg))   # leaves of their own
    cell, centre = R.cell_distance(p, obj_shape, m.to(dtype), f, eps)
    gp, gf = torch.autograd.grad(cell, [p, f], retain_graph=True)
    gpc, = torch.autograd.grad(centre, [p])
    return cell.detach(), centre.detach(), gp, gf, gpc


_cell_refs = {}


def cell_refs(pose, fg, m, obj_shape, eps):
    """``ref_cell`` in fp32 and fp64, once per operands (keyed on their bytes and shapes) and eps."""
    key = (tuple(obj_shape), float(eps)) + tuple(
        (tuple(x.shape), hashlib.sha1(x.detach().contiguous().numpy().tobytes()).digest()) for x in (pose, fg, m))
    if key not in _cell_refs:
        _cell_refs[key] = (ref_cell(pose, fg, m, obj_shape, eps, torch.float32),
                           ref_cell(pose, fg, m, obj_shape, eps, torch.float64))
    return _cell_refs[key]


def chosen_objects(pose, fg, m, obj_shape, eps):
    """The object the fp64 restatement chooses per pixel, (B T, H W): argmin of (mask + eps)(1 - fg) obj_cell_dis."""
    from waldo_amd.tools.utils import get_grid
    h, w = m.shape[-2:]
    p = pose.double()
    g = p.view(*p.shape[:3], *obj_shape, 2)
    cell = ((g[:, :, :, 1:, 1:] + g[:, :, :, 1:, :-1] + g[:, :, :, :-1, 1:] + g[:, :, :, :-1, :-1]) / 4)
    cell = cell.reshape(-1, p.shape[2], (obj_shape[0] - 1) * (obj_shape[1] - 1), 1, 2)
    grid = get_grid(h, w).double().view(1, 1, 1, -1, 2)
    dis = ((cell - grid) ** 2).sum(-1).sum(2)                                          # (F, No, HW)
    wgt = ((m.double() + eps) * (1 - fg.double())).view(-1, 1, h * w)
    return (wgt * dis).argmin(dim=1)


@functools.lru_cache(maxsize=None)
def blur_input(h, w):
    return torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(1000 * h + w))


@functools.lru_cache(maxsize=None)
def blur_refs(h, w, k, sigma):
    x = blur_input(h, w)
    return R.gaussian_blur(x, sigma, k), R.gaussian_blur(x.double(), sigma, k)


@functools.lru_cache(maxsize=None)
def edge_input(h, w):
    return 0.03 * torch.randn(2, 2, h, w, generator=torch.Generator().manual_seed(h + w))
