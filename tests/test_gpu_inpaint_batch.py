"""``WIF.inpaint`` on a batch of clips with the default option set (loop_ii, shadows, propagate_obj): the objects that
enter through the left / right border are chosen per clip ON THE DEVICE (csrc/border_objects.hip), the polygon test
reads its corners there (``waldo_points_in_polygon_dev_fwd``) and the object flow takes one object id per clip.

    * the selection kernel against the torch expressions of models/nets/wif.py:135-157, per clip, bit for bit;
    * the device polygon test against the host-corner form (itself pinned to matplotlib in tests/test_inpaint.py);
    * one batched call against one-clip calls of the untouched B = 1 path, ``torch.equal`` per clip;
    * every clip against the CPU oracle, by the rule of ``test_inpaint_hip_vs_oracle_and_reference``;
    * ``always_inpaint_borders``: no device -> host read, and the call replays from a HIP graph."""
import types

import pytest
import torch

from oracle import inpaint_oracle as IO
from oracle import warper_oracle as WO
from oracle import wif_oracle as O
from oracle.make_golden import inpaint_inputs, inpaint_opt
from test_inpaint import flipped_fraction, make_forward, warper_opt  # tests/test_inpaint.py

pytestmark = pytest.mark.gpu

CTX_LEN = 2


# ------------------------------------------------------------------------------------------------ selection kernel
def torch_border_objects(pred_flow, ident, alpha_ctx):
    """wif.py:135-157 with framework ops on the device, one clip at a time (the expressions of ``WIF._border_objects``):
    pred_flow (B, 2, H, W), ident (1, H, W, 2), alpha_ctx (B, Tc, Tp, L, H, W)."""
    h, w = ident.shape[1:3]
    border = 3
    nb = alpha_ctx.shape[0]
    valid = torch.zeros(nb, 2, dtype=torch.int32)
    obj_id = torch.zeros(nb, 2, dtype=torch.int64)
    corners = torch.zeros(nb, 2, 4, 2, dtype=torch.float64)
    counts = torch.zeros(nb, 2, alpha_ctx.shape[3] - 1)

    def to_px(g):
        return torch.stack([(g[..., 0] * w + w - 1) / 2, (g[..., 1] * h + h - 1) / 2], dim=-1)

    orig_px = to_px(ident)
    for b in range(nb):
        pred_px = to_px(pred_flow[b:b + 1].permute(0, 2, 3, 1) + ident)
        all_obj = (((alpha_ctx[b:b + 1, :, -1, 1:] + 1) / 2).max(dim=1)[0] > 0.9).float()
        for s, at_border in enumerate((pred_px[..., 0] < border, pred_px[..., 0] >= w - border)):
            hit = at_border.float().unsqueeze(1) * all_obj
            counts[b, s] = hit.flatten(start_dim=2).sum(-1)[0].cpu()
            if not hit.sum() > 0:
                continue
            oid = int(hit.flatten(start_dim=2).sum(-1).argmax(dim=1)[0])
            sel = hit[:, oid].bool()
            bv, ov = pred_px[sel], orig_px[sel]
            by0, by1, ox0, ox1, oy0, oy1 = torch.stack([bv[:, 1].min(), bv[:, 1].max(), ov[:, 0].min(), ov[:, 0].max(),
                                                        ov[:, 1].min(), ov[:, 1].max()]).tolist()
            if s == 0:
                c = [(0, by0), (0, by1), (ox1, oy1), (ox1, oy0)]
            else:
                c = [(ox0, oy0), (ox0, oy1), (w - 1, by1), (w - 1, by0)]
            valid[b, s], obj_id[b, s] = 1, oid
            corners[b, s] = torch.tensor(c, dtype=torch.float64)
    return valid, obj_id, corners, counts


ALPHA_EXACT = float(torch.tensor(0.9) * 2 - 1)  # (a + 1) / 2 == float32(0.9) exactly: at the threshold, not above it
KINDS = ("left", "both", "none", "tie", "exact")


def selection_inputs(kinds, tc, nl, h, w, seed):
    """Clips of the given kinds: background alphas below the threshold everywhere, blocks of 0.95 where an object is;
    a random flow of about a pixel, so that the `at` tests cut through the columns next to the borders."""
    g = torch.Generator().manual_seed(seed)
    nb, tp = len(kinds), 2
    actx = torch.rand(nb, tc, tp, nl, h, w, generator=g) * 1.6 - 1.0            # (a + 1) / 2 < 0.8
    flow = (torch.rand(nb, tc, tp, 2, h, w, generator=g) - 0.5) * (4.0 / w)
    r0, r1 = h // 4, h // 4 + h // 3
    last = nl - 1                                                               # object ids 0 and nl - 2 are used
    for b, kind in enumerate(kinds):
        a = actx[b, :, -1]
        if kind in ("left", "both"):
            a[tc - 1, last, r0:r1, 0:5] = 0.95                                  # (in one context only: the max finds it)
            flow[b, -1, -1, 0, r0:r1, 0:5] = -0.1
        if kind == "both":
            a[0, 1, r0 + 2:r1 + 3, w - 5:w] = 0.95
            flow[b, -1, -1, 0, r0 + 2:r1 + 3, w - 5:w] = 0.1
        if kind == "tie":                                                        # two objects, equal counts: the lowest id
            a[:, last, 2:8, 0:3] = 0.95
            a[:, 1, 10:16, 0:3] = 0.95
            flow[b, -1, -1, 0, :, 0:3] = -0.1
        if kind == "exact":                                                      # a large object AT 0.9, a small one above
            a[:, 1, :, 0:4] = ALPHA_EXACT
            a[0, last, 3:6, 0:2] = 0.95
            flow[b, -1, -1, 0, :, 0:4] = -0.1
    return flow, actx


@pytest.mark.parametrize("h,w,nl,tc,kinds", [(32, 64, 3, 1, ("left", "both", "none")),
                                             (33, 50, 7, 4, ("tie", "exact", "left")),
                                             (40, 72, 18, 4, ("both", "tie", "exact")),
                                             (33, 50, 18, 1, ("none", "exact", "both")),
                                             (40, 72, 7, 1, ("tie", "none", "left"))])
def test_selection_kernel_gives_the_torch_expressions(dev, h, w, nl, tc, kinds):
    """``waldo_border_objects_fwd`` against wif.py:135-157 evaluated per clip with framework ops: ``valid``, ``obj_id``
    and the float64 corners EQUAL, for rasters that are no multiple of the 256-pixel tile, 2 / 6 / 17 objects, one and
    four contexts, B = 3 clips of every kind (an object at the left border; at both; at none; two objects with equal
    counts -- the lowest id wins, as torch.argmax; an object whose alpha is 0.9 exactly, not above), a contiguous
    ``alpha_ctx`` and the strided raw-slot view ``decode_output`` returns (read in place: no copy)."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.utils import get_grid
    flow, dense = selection_inputs(kinds, tc, nl, h, w, seed=h + w + nl)
    ident = get_grid(h, w).to(dev)
    flow = flow.to(dev)
    pf = flow[:, -1, -1]
    nb, _, tp = dense.shape[:3]
    big = torch.zeros(nb, tp, tc, nl + 7, h, w)
    big[:, :, :, 7:] = dense.permute(0, 2, 1, 3, 4, 5)
    view = big.to(dev)[:, :, :, 7:].permute(0, 2, 1, 3, 4, 5)
    assert torch.equal(view.cpu(), dense) and not view.is_contiguous()
    want_valid, want_id, want_corners, counts = torch_border_objects(pf, ident, dense.to(dev))
    for b, kind in enumerate(kinds):  # (the inputs are of the kind they claim to be)
        assert want_valid[b].tolist() == {"left": [1, 0], "both": [1, 1], "none": [0, 0], "tie": [1, 0], "exact": [1, 0]}[kind]
        if kind == "tie":
            assert counts[b, 0, 0] == counts[b, 0, nl - 2] > 0 and want_id[b, 0] == 0
        if kind == "exact":
            assert want_id[b, 0] == nl - 2 and counts[b, 0, 0] == 0
            assert (torch.tensor(ALPHA_EXACT) + 1) / 2 == torch.tensor(0.9)
    for actx in (dense.to(dev), view):
        valid, obj_id, corners = WF.border_objects(pf, ident, actx)
        assert valid.dtype == torch.int32 and obj_id.dtype == torch.int64 and corners.dtype == torch.float64
        assert torch.equal(valid.cpu(), want_valid), (valid.cpu(), want_valid)
        assert torch.equal(obj_id.cpu(), want_id), (obj_id.cpu(), want_id)
        assert torch.equal(corners.cpu(), want_corners), (corners.cpu() - want_corners).abs().max()


def test_selection_kernel_full_raster_and_large_counts(dev):
    """512 x 1024, B = 2, two contexts, 12 layers, one predicted frame (a 100 MB ``alpha_ctx`` generated on the device):
    2048 workgroups per clip, counts above 2^16 (a 200-column band leaves through the left border), a second, smaller
    object at the same border and one at the right border of the other clip."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.utils import get_grid
    h, w, nb, tc, nl = 512, 1024, 2, 2, 12
    g = torch.Generator(device=dev).manual_seed(5)
    actx = torch.rand(nb, tc, 1, nl, h, w, generator=g, device=dev) * 1.6 - 1.0
    flow = (torch.rand(nb, 2, h, w, generator=g, device=dev) - 0.5) * (4.0 / w)
    actx[0, 1, 0, 4, :, 0:200] = 0.95
    actx[0, 0, 0, 9, 100:300, 0:150] = 0.95
    flow[0, 0, :, 0:200] = -0.4
    actx[1, 0, 0, 11, 37:411, 1000:1024] = 0.95
    flow[1, 0, 37:411, 1000:1024] = 0.05
    ident = get_grid(h, w).to(dev)
    want_valid, want_id, want_corners, counts = torch_border_objects(flow, ident, actx)
    assert counts[0, 0, 3] > 2 ** 16 and counts[0, 0, 8] > 0 and want_valid.tolist() == [[1, 0], [0, 1]]
    assert want_id.tolist() == [[3, 0], [0, 10]]
    valid, obj_id, corners = WF.border_objects(flow, ident, actx)
    assert torch.equal(valid.cpu(), want_valid) and torch.equal(obj_id.cpu(), want_id)
    assert torch.equal(corners.cpu(), want_corners), (corners.cpu() - want_corners).abs().max()


def test_selection_kernel_lets_a_nan_through(dev):
    """A NaN among the selected pixels' coordinates gives NaN extrema, as ``torch.min`` / ``torch.max``; a NaN alpha wins
    the maximum over the contexts and is then not above 0.9; a NaN x coordinate is at no border."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.utils import get_grid
    h, w, nl, tc = 32, 64, 3, 2
    flow, actx = selection_inputs(("left", "both", "left"), tc, nl, h, w, seed=2)
    flow[0, -1, -1, 1, 10, 1] = float("nan")            # y of a selected pixel: by0, by1 are NaN
    actx[1, 0, -1, nl - 1, 12, 0:5] = float("nan")      # hides the 0.95 of the other context in this row
    flow[2, -1, -1, 0, 9, 0:5] = float("nan")           # this row is not at the border
    ident = get_grid(h, w).to(dev)
    pf = flow.to(dev)[:, -1, -1]
    want_valid, want_id, want_corners, _ = torch_border_objects(pf, ident, actx.to(dev))
    valid, obj_id, corners = WF.border_objects(pf, ident, actx.to(dev))
    assert torch.isnan(want_corners[0, 0, :2, 1]).all() and torch.isnan(want_corners).sum() == 2
    assert torch.equal(valid.cpu(), want_valid) and torch.equal(obj_id.cpu(), want_id)
    assert torch.equal(torch.isnan(corners.cpu()), torch.isnan(want_corners))
    assert torch.equal(corners.cpu().nan_to_num(-7.0), want_corners.nan_to_num(-7.0))


# ------------------------------------------------------------------------------------------------ polygon test
def test_device_polygon_test_gives_the_host_forms_answers(dev):
    """``waldo_points_in_polygon_dev_fwd`` (corners and validity in device memory, P polygons per launch) against
    ``WF.points_in_polygon`` with the same corners on the host -- the form tests/test_inpaint.py pins to matplotlib --
    for random convex, self-intersecting and lattice polygons of 3 ... 16 corners (repeated and collinear corners among
    them), random points and points ON vertices, edges and the lattice: every answer equal.  An invalid polygon and
    a path of fewer than three corners contain nothing; float32 corners are widened exactly; a strided table of corners
    is read in place."""
    import numpy as np
    from waldo_amd import functional as WF
    rng = np.random.default_rng(21)
    total = 0
    for k in (3, 4, 5, 9, 16):
        polys = []
        for case in range(6):
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = rng.uniform(0.2, 1.0, k) * rng.choice([10.0, 300.0])
            poly = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1) + rng.uniform(-50, 50, 2)
            if case % 3 == 0:
                poly = poly[rng.permutation(k)]                  # self-intersecting
            if case % 2 == 0:
                poly = np.round(poly)                            # lattice corners: horizontal / vertical / repeated ones
            if case == 4 and k > 3:
                poly[1] = poly[0]                                # a repeated corner
                poly[3] = (poly[2] + poly[(4) % k]) / 2          # a collinear one
            polys.append(poly.astype(np.float32).astype(np.float64))
        allp = np.concatenate(polys)
        lo, hi = allp.min(0) - 5, allp.max(0) + 5
        pts = [rng.uniform(lo, hi, (6000, 2)), allp, np.round(rng.uniform(lo, hi, (3000, 2)))]
        for poly in polys:
            pts.append((poly + np.roll(poly, 1, 0)) / 2)
            for t in (0.25, 0.125):
                pts.append(poly * t + np.roll(poly, -1, 0) * (1 - t))
        pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(pts), dtype=np.float32)).to(dev)
        want = torch.stack([WF.points_in_polygon(pts, [(float(x), float(y)) for x, y in poly]) for poly in polys])
        cn = torch.from_numpy(np.stack(polys)).to(dev)
        got = WF.points_in_polygon(pts, cn)
        assert got.shape == want.shape and got.dtype == torch.bool
        assert torch.equal(got, want), (k, (got != want).sum().item())
        assert 0.02 < want.float().mean() < 0.98
        valid = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.int32, device=dev)
        masked = WF.points_in_polygon(pts, cn, valid=valid)
        assert torch.equal(masked, want & (valid.view(-1, 1) != 0)) and not masked[1].any() and not masked[4].any()
        assert torch.equal(WF.points_in_polygon(pts, cn, valid=valid.bool()), masked)
        assert torch.equal(WF.points_in_polygon(pts, cn.float()), want)              # (the corners are float32 values)
        assert torch.equal(WF.points_in_polygon(pts, cn[2]), want[2])                # one polygon, (K, 2)
        table = torch.zeros(6, 2, k, 2, dtype=torch.float64, device=dev)             # a (P, 2, K, 2) table, one side of it
        table[:, 1] = cn
        vt = torch.stack([1 - valid, valid], dim=1)
        assert torch.equal(WF.points_in_polygon(pts, table[:, 1], valid=vt[:, 1]), masked)
        total += want.numel()
    pts = torch.rand(500, 2, device=dev) * 8
    assert not WF.points_in_polygon(pts, torch.tensor([[[0.0, 0.0], [8.0, 0.0]]], dtype=torch.float64, device=dev)).any()
    tri = torch.tensor([[0.0, 0.0], [8.0, 0.0], [8.0, 8.0]], dtype=torch.float64, device=dev)
    odd = torch.tensor([[float("nan"), 1.0], [2.0, float("inf")], [6.0, 2.0]], device=dev)
    assert WF.points_in_polygon(odd, tri).tolist() == [False, False, True]           # non-finite points are outside
    grid_pts = torch.rand(2, 5, 7, 2, device=dev) * 8                                # any leading shape
    assert WF.points_in_polygon(grid_pts, tri.unsqueeze(0)).shape == (1, 2, 5, 7)
    assert total > 250_000


# ------------------------------------------------------------------------------------------------ the batched call
class LoopConv(torch.nn.Module):
    """The 1 x 1 convolution that stands in for the UNet, spelled as a chain of elementwise operations: its result for a
    frame cannot depend on how many frames share the call (a library convolution may pick another algorithm)."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(weight.clone(), requires_grad=False)
        self.bias = torch.nn.Parameter(bias.clone(), requires_grad=False)

    def forward(self, x):
        out = self.bias.view(1, -1, 1, 1) + self.weight[:, 0].view(1, -1, 1, 1) * x[:, 0:1]
        for c in range(1, x.shape[1]):
            out = out + self.weight[:, c].view(1, -1, 1, 1) * x[:, c:c + 1]
        return out


def stub_inpainter(img, mask, **kw):
    """``IO.stub_inpainter`` clip by clip.  ``WIF.inpaint`` on a batch asks of its inpainter that the clips of a batch do
    not influence each other; the oracle's stub takes a mean over each clip's pixels with a framework reduction, whose
    block shape -- and with it the order of the sum, the last bit of the mean -- depends on how many clips share the
    call (measured at 32 x 64: one value of clip 0 moved by 1.5e-8 between B = 1 and B = 5).  Called on one clip at a
    time it is the same function of a clip whatever the batch."""
    return torch.cat([IO.stub_inpainter(img[b:b + 1], mask[b:b + 1], **kw) for b in range(img.shape[0])])


def five_clips():
    """Five clips of ``oracle.make_golden.inpaint_inputs`` (32 x 64, 2 objects, 2 + 2 frames), edited as
    ``recipe_inpaint_inputs`` edits its inputs: an object at the left border (seed 9, as generated); at both borders
    (33); at none (45); two objects with equal counts at the left border (57); object 2 alone at the left border (9)."""
    def blank(d):  # the generated object at the left border, taken out again
        d["alpha_ctx"][:, :, -1, 1, 8:20, 0:5] = -0.9
        return d

    left = inpaint_inputs(O.get_grid, 9)
    both = inpaint_inputs(O.get_grid, 33)
    both["alpha_ctx"][:, :, -1, 2, 10:24, 59:64] = 0.95
    both["pred_flow"][:, -1, -1, 0, 10:24, 59:64] = 0.1
    none = blank(inpaint_inputs(O.get_grid, 45))
    tie = blank(inpaint_inputs(O.get_grid, 57))
    for layer, rows in ((1, slice(4, 10)), (2, slice(16, 22))):
        tie["alpha_ctx"][:, :, -1, layer, rows, 0:5] = 0.95
        tie["pred_flow"][:, -1, -1, 0, rows, 0:5] = -0.1
    second = blank(inpaint_inputs(O.get_grid, 9))
    second["alpha_ctx"][:, :, -1, 2, 6:18, 0:5] = 0.95
    second["pred_flow"][:, -1, -1, 0, 6:18, 0:5] = -0.1
    return [left, both, none, tie, second]


WANT_SIDES = [[1, 0], [1, 1], [0, 0], [1, 0], [1, 0]]
WANT_IDS = [[0, 0], [0, 1], [0, 0], [0, 0], [1, 0]]
KEYS = ("raw_output", "alpha", "alpha_ctx", "real_vid", "pred_flow")


@pytest.fixture(scope="module")
def scene(dev):
    """The five clips, the oracle's grids for each (computed once, on the CPU), the stand-in network, and on the device:
    the batch, the modules, and the one-clip results of the untouched B = 1 path for both propagation forms."""
    from waldo_amd.nets import WIF, Warper
    clips = five_clips()
    wopt = warper_opt()
    cfg = WO.WarperCfg.from_opt(wopt)
    opt = inpaint_opt()
    for k, v in vars(wopt).items():
        setattr(opt, k, v)
    with torch.no_grad():
        grids = [WO.warper_grids(cfg, d["obj_pose"], d["bg_pose"]) for d in clips]
    gw = torch.Generator().manual_seed(10)
    net = dict(weight=torch.randn(5, clips[0]["channels"], 1, 1, generator=gw) * 0.3, bias=torch.randn(5, generator=gw) * 0.1)
    wif = WIF(opt, unet=LoopConv(net["weight"], net["bias"])).to(dev)
    warper = Warper(wopt).to(dev)
    batch = {k: torch.cat([d[k] for d in clips]).to(dev) for k in KEYS}
    grid = [torch.cat([g[i] for g in grids]).to(dev) for i in range(4)]
    s = types.SimpleNamespace(clips=clips, grids=grids, cfg=cfg, opt=opt, net=net, wif=wif, warper=warper, batch=batch,
                              grid=grid, n=len(clips))

    def run(sel=slice(None), inpainter=stub_inpainter):
        with torch.no_grad():
            return wif.inpaint(inpainter, *(batch[k][sel] for k in KEYS), CTX_LEN, warper, [g[sel] for g in grid])

    s.run = run
    s.single = {}
    for fuse in (True, False):
        wif.fuse_propagate = fuse
        s.single[fuse] = [run(slice(b, b + 1)) for b in range(s.n)]
    wif.fuse_propagate = True
    return s


@pytest.fixture(autouse=True)
def default_switches(request):
    yield
    if "scene" in request.fixturenames:
        wif = request.getfixturevalue("scene").wif
        wif.fuse_propagate, wif.border_on_device, wif.always_inpaint_borders = True, None, False


def test_the_five_clips_hit_the_intended_sides(dev, scene):
    """The selection on the five clips: sides, object ids (the tie resolves to object 0) and the hit counts 60 / 60 + 70 /
    0 / 30 : 30 / 60 -- and the one-clip results differ from each other where the border objects differ."""
    from waldo_amd import functional as WF
    pf = scene.batch["pred_flow"][:, -1, -1]
    valid, obj_id, corners = WF.border_objects(pf, scene.wif.src_grid_hd, scene.batch["alpha_ctx"])
    assert valid.tolist() == WANT_SIDES and obj_id.tolist() == WANT_IDS
    want_valid, want_id, want_corners, counts = torch_border_objects(pf, scene.wif.src_grid_hd, scene.batch["alpha_ctx"])
    assert torch.equal(valid.cpu(), want_valid) and torch.equal(obj_id.cpu(), want_id) and torch.equal(corners.cpu(), want_corners)
    assert counts[:, 0].tolist() == [[60, 0], [60, 0], [0, 0], [30, 30], [0, 60]]
    assert counts[:, 1].tolist() == [[0, 0], [0, 70], [0, 0], [0, 0], [0, 0]]
    assert not torch.equal(scene.single[True][0], scene.single[True][4])


@pytest.mark.parametrize("always", [False, True])
@pytest.mark.parametrize("fuse", [True, False])
def test_batched_call_equals_the_one_clip_calls(dev, scene, fuse, always):
    """ONE ``wif.inpaint`` on the five clips with the default option set against five one-clip calls of the B = 1 path (the
    reference's branch: host reads, host corners) on the same grids: ``torch.equal`` per clip, for the fused propagation
    step and the spelled-out loop, with the one host read and without any (``always_inpaint_borders``).  (The parent
    commit raises here: its border-object branch is one clip only.)"""
    from waldo_amd import _lib
    wif = scene.wif
    wif.fuse_propagate, wif.always_inpaint_borders = fuse, always
    with _lib.KernelTimer() as kt:
        out = scene.run()
        torch.cuda.synchronize()
    launched = kt.summary()
    assert launched["waldo_border_objects_fwd"][0] == 1 and launched["waldo_points_in_polygon_dev_fwd"][0] == 2
    assert "waldo_points_in_polygon_fwd" not in launched and ("waldo_inpaint_propagate_fwd" in launched) == fuse
    assert out.shape == (scene.n, CTX_LEN + 2, 3, 32, 64) and torch.isfinite(out).all()
    for b in range(scene.n):
        one = scene.single[fuse][b]
        assert torch.equal(out[b:b + 1], one), (b, fuse, always, (out[b:b + 1] - one).abs().max().item())
    assert torch.equal(scene.single[True][1], scene.single[False][1])


def test_one_side_only_skips_the_other_sides_inpainter(dev, scene):
    """Clips 0, 2, 3 (left, none, tie): nothing enters on the right, so with the host read the right side is skipped as
    the reference skips it -- one polygon launch -- and without it both run; the frames are the same."""
    from waldo_amd import _lib
    sel = [0, 2, 3]
    outs = []
    for always, launches in ((False, 1), (True, 2)):
        scene.wif.always_inpaint_borders = always
        with _lib.KernelTimer() as kt:
            outs.append(scene.run(sel))
            torch.cuda.synchronize()
        assert kt.summary()["waldo_points_in_polygon_dev_fwd"][0] == launches
    assert torch.equal(outs[0], outs[1])
    for i, b in enumerate(sel):
        assert torch.equal(outs[0][i:i + 1], scene.single[True][b])
    scene.wif.always_inpaint_borders = False
    with _lib.KernelTimer() as kt:  # no clip has a border object: no polygon, no inpainter call for the borders
        nothing = scene.run([2, 2])
        torch.cuda.synchronize()
    assert "waldo_points_in_polygon_dev_fwd" not in kt.summary()
    assert torch.equal(nothing[:1], scene.single[True][2]) and torch.equal(nothing[1:], scene.single[True][2])


def test_device_path_for_one_clip_equals_the_default_path(dev, scene):
    """``border_on_device = True`` at B = 1 against the default (host-read) path: the same frames for every clip, and the
    default path itself launches what it launched before (the host-corner polygon test, no selection kernel)."""
    from waldo_amd import _lib
    wif = scene.wif
    for fuse in (True, False):
        wif.fuse_propagate = fuse
        for b in range(scene.n):
            wif.border_on_device = True
            with _lib.KernelTimer() as kt:
                got = scene.run(slice(b, b + 1))
                torch.cuda.synchronize()
            assert kt.summary()["waldo_border_objects_fwd"][0] == 1
            assert torch.equal(got, scene.single[fuse][b]), (b, fuse)
    wif.fuse_propagate, wif.border_on_device = True, None
    with _lib.KernelTimer() as kt:
        again = scene.run(slice(1, 2))
        torch.cuda.synchronize()
    launched = kt.summary()
    assert launched["waldo_points_in_polygon_fwd"][0] == 2 and "waldo_border_objects_fwd" not in launched
    assert "waldo_points_in_polygon_dev_fwd" not in launched and torch.equal(again, scene.single[True][1])
    wif.border_on_device = False  # today's behaviour for a batch too: the one-clip branch, which cannot index a batch
    with pytest.raises(Exception):
        scene.run()


@pytest.mark.parametrize("fuse", [True, False])
def test_a_clip_without_an_object_ignores_what_the_inpainter_returned(dev, scene, fuse):
    """An inpainter that answers NaN for every clip whose border region is empty: those clips' frames, and the other
    clips, are what they are with the stub -- the slot of a clip with no object at a side is neutral in the fused step
    and in the spelled-out loop."""
    wif = scene.wif
    wif.fuse_propagate, wif.always_inpaint_borders = fuse, True
    inside, poisoned = [False], [0]

    def inpainter(img, mask, **kw):
        out = stub_inpainter(img, mask, **kw)
        if inside[0]:
            empty = mask.flatten(1).sum(dim=1) == 0
            poisoned[0] += 1
            out = torch.where(empty.view(-1, 1, 1, 1), torch.full_like(out, float("nan")), out)
        return out

    border = wif._border_objects

    def watched(*a, **kw):
        inside[0] = True
        try:
            return border(*a, **kw)
        finally:
            inside[0] = False

    wif._border_objects = watched
    try:
        out = scene.run(inpainter=inpainter)
    finally:
        del wif._border_objects
    assert poisoned[0] == 2 and torch.isfinite(out).all()
    for b in range(scene.n):
        assert torch.equal(out[b:b + 1], scene.single[fuse][b]), (b, fuse)


@pytest.mark.parametrize("clip", range(5))
def test_batched_clips_against_the_cpu_oracle(dev, scene, clip):
    """Clip b of the batched call against ``IO.wif_inpaint`` on the clip alone with the oracle's grids, by the rule of
    ``test_inpaint_hip_vs_oracle_and_reference``: at most 2e-3 of the values off by more than 1e-4, and those at pixels
    the oracle itself flips under 3e-5 input noise.  (The batched result equals the one-clip product result bit for
    bit -- the test above -- so this is a check of the new clips, not a new tolerance.)"""
    d, grid = scene.clips[clip], scene.grids[clip]
    with torch.no_grad():
        ref = IO.wif_inpaint(scene.opt, scene.cfg, make_forward(scene.net), IO.stub_inpainter, d["raw_output"].clone(),
                             d["alpha"], d["alpha_ctx"], d["real_vid"], d["pred_flow"], CTX_LEN, grid)
    out = scene.run()[clip:clip + 1]
    assert out.shape == ref.shape
    frac = flipped_fraction(out, ref)
    diff = (out.detach().cpu().double() - ref.double()).abs()
    flipped = diff > 1e-4
    print(f"[inpaint batch, clip {clip}] flipped {frac:.2e}; max error of the other values {diff[~flipped].max().item():.2e}")
    assert frac <= 2e-3, f"clip {clip}: {frac:.2e} of the values differ from the oracle by more than 1e-4"
    if flipped.any():
        unstable = torch.zeros_like(flipped)
        for seed in range(4):
            gen = torch.Generator().manual_seed(seed)

            def jig(t):
                return t + 3e-5 * torch.randn(t.shape, generator=gen)
            with torch.no_grad():
                pert = IO.wif_inpaint(scene.opt, scene.cfg, make_forward(scene.net), IO.stub_inpainter, jig(d["raw_output"]),
                                      jig(d["alpha"]), jig(d["alpha_ctx"]), d["real_vid"], jig(d["pred_flow"]), CTX_LEN, grid)
            unstable |= (pert.double() - ref.double()).abs() > 1e-4
        near = torch.nn.functional.max_pool2d(unstable.any(dim=-3, keepdim=True).float().flatten(0, -4), 5, 1, 2)
        near = near.view(*unstable.shape[:-3], 1, *unstable.shape[-2:]).bool().expand_as(flipped)
        inside = (flipped & near).sum().item() / flipped.sum().item()
        print(f"[inpaint batch, clip {clip}] {inside:.0%} of the flipped values lie where the oracle flips under 3e-5 "
              f"input noise ({unstable.double().mean().item():.2e} of all values)")
        assert inside >= 0.9, f"clip {clip}: only {inside:.0%} of the flipped values are at noise-unstable pixels"


# ------------------------------------------------------------------------------------------------ no host read
def test_no_host_read_with_always_inpaint_borders(dev, scene):
    """``always_inpaint_borders``: the batched call makes no device -> host read -- it runs under
    ``torch.cuda.set_sync_debug_mode("error")``, in which a synchronising call raises (shown first on an ``.item()``, and
    on the call WITH the host read) -- and the same frames come out."""
    wif = scene.wif
    want = scene.run()
    wif.always_inpaint_borders = True
    scene.run()  # (allocator and lazy initialisation outside the watched call)
    probe = torch.ones(1, device=dev)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        got = scene.run()
        wif.always_inpaint_borders = False
        with pytest.raises(RuntimeError):
            scene.run()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got, want)


def test_batched_call_replays_from_a_hip_graph(dev, scene):
    """The batched call with ``always_inpaint_borders`` captured by ``waldo_amd.graphs.GraphedCall`` (stub inpainter): the
    replay equals the eager result, also for other inputs of the same shapes -- the clips in another order, so every
    per-clip decision (sides, object ids, corners) is taken anew on the device inside the graph."""
    from waldo_amd.graphs import GraphedCall
    wif, warper = scene.wif, scene.warper
    wif.always_inpaint_borders = True
    want = scene.run().clone()
    order = [3, 1, 4, 0, 2]
    want_other = scene.run(order).clone()

    def fn(raw_output, alpha, alpha_ctx, real_vid, pred_flow, tgo, sgo, tgb, sgb):
        return wif.inpaint(stub_inpainter, raw_output, alpha, alpha_ctx, real_vid, pred_flow, CTX_LEN, warper,
                           [tgo, sgo, tgb, sgb])

    args = [scene.batch[k] for k in KEYS] + list(scene.grid)
    graphed = GraphedCall(fn, *args)
    assert torch.equal(graphed(*args), want)
    assert torch.equal(graphed(*(a[order] for a in args)), want_other)
    assert torch.equal(graphed(*args), want)
    graphed.check()
