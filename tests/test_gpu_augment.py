"""GPU: the clip augmentation kernel (waldo_amd.augment, include/waldo_hip.h "Clip augmentation") against its restatement
in torch ops (tests/augment_ref.py) and against itself: identity, crop edges, flips, the two-stage flow, the clamping of
the tables, the launch count, graph capture and the Augmenter.  The shapes are the smallest that exercise the index
arithmetic: a 20 x 68 clip, outputs 20 x 68 (four pixels per lane, two workgroups per frame) and 23 x 70 (one pixel per
lane, odd sizes, rows that straddle workgroups)."""
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R
from parity import TOL, close

pytestmark = pytest.mark.gpu

B, T, HD, WD, NL = 2, 3, 20, 68, 5
FULL = (0, 0, HD, WD)
CORNER = (7, 41, 13, 27)  # touches the bottom-right corner
BOXES = {"full+corner": (FULL, CORNER), "pixel+odd": ((0, 0, 1, 1), (3, 5, 13, 40))}  # 13 -> 23: a non-dyadic ratio
# all six orders and 255 across the frames
ORDERS = {"a": ((0, 1, 2), (3, 4, 5)), "b": ((255, 5, 3), (1, 255, 0))}
JITTER = ((0.5, 1.5, 0.25), (1.5, 0.5, -0.25))  # the ends of --colorjitter 0.5
ZOOM = (1.25, 1.0625)


def clip_bytes(seed=0, b=B):
    """Random bytes; class bytes in 0..4 and some 7 and 255 (both >= Nl); frame (0, 1) grey (max == min at every pixel);
    frame (b-1, 2) with bytes 0 and 255 in every combination that matters to the hue."""
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (b, T, HD, WD, 4), generator=g, dtype=torch.uint8)
    cls = torch.randint(0, NL + 2, (b, T, HD, WD), generator=g)
    data[..., 3] = torch.where(cls == NL, 7, torch.where(cls == NL + 1, 255, cls)).to(torch.uint8)
    data[0, 1, :, :, 1] = data[0, 1, :, :, 0]
    data[0, 1, :, :, 2] = data[0, 1, :, :, 0]
    ends = torch.tensor([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 255], [0, 0, 255], [255, 255, 0]],
                        dtype=torch.uint8)
    data[b - 1, 2, 8:10, 42:48, :3] = ends
    data[b - 1, 2, 0, :6, :3] = ends
    return data


def make_params(boxes, flips, orders=ORDERS["a"], jitter=JITTER, zoom=ZOOM):
    from waldo_amd import augment as A
    return A.AugmentParams(torch.tensor(boxes, dtype=torch.int32), torch.tensor(flips, dtype=torch.uint8),
                           torch.tensor(jitter, dtype=torch.float32), torch.tensor(orders, dtype=torch.uint8),
                           torch.tensor(zoom, dtype=torch.float32))


def make_flow(shape, seed=1, b=B):
    return None if shape is None else 0.1 * torch.randn(b, T, 2, *shape, generator=torch.Generator().manual_seed(seed))


def run(dev, data, params, flow=None, out_size=None, nl=NL):
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    out, fl = A.augment_clip(WF.PackedClip(data.to(dev), nl), params.to(dev),
                             flow=None if flow is None else flow.to(dev), out_size=out_size)
    torch.cuda.synchronize()
    return out, fl


def compare(got, data, params, flow, out_size, what, nl=NL):
    """The kernel against the restatement in fp32, with the restatement's own distance to fp64 as its noise: RGB, layout
    and flow planes separately.  Nothing is exempt: taps, hue sectors and clamps are all continuous."""
    ref32 = R.augment_ref(data, nl, params, flow, out_size, torch.float32)
    ref64 = R.augment_ref(data, nl, params, flow, out_size, torch.float64)
    assert got[0].dtype == torch.float32 and got[0].shape == ref32[0].shape
    close(got[0][:, :, :3], ref32[0][:, :, :3], exact=ref64[0][:, :, :3], what=f"{what} rgb")
    close(got[0][:, :, 3:], ref32[0][:, :, 3:], exact=ref64[0][:, :, 3:], what=f"{what} layout")
    if flow is None:
        assert got[1] is None
    else:
        close(got[1], ref32[1], exact=ref64[1], rel=True, what=f"{what} flow")
    return ref64


CASES = [((20, 68), None, "full+corner", (1, 0), "a"), ((23, 70), (8, 27), "full+corner", (0, 2), "b"),
         ((23, 70), (20, 68), "pixel+odd", (3, 0), "a"), ((20, 68), (8, 27), "pixel+odd", (0, 1), "b"),
         ((20, 68), (20, 68), "full+corner", (2, 1), "a"), ((23, 70), None, "pixel+odd", (0, 3), "b")]


@pytest.mark.parametrize("out_size,flow_shape,boxes,flips,orders", CASES,
                         ids=[f"{c[0][0]}x{c[0][1]}-flow{c[1]}-{c[2]}-flip{c[3][0]}{c[3][1]}-{c[4]}".replace(" ", "")
                              for c in CASES])
def test_kernel_against_the_restatement(dev, out_size, flow_shape, boxes, flips, orders):
    data, flow = clip_bytes(), make_flow(flow_shape)
    params = make_params(BOXES[boxes], flips, ORDERS[orders])
    got = run(dev, data, params, flow, out_size)
    compare(got, data, params, flow, out_size, f"{out_size} {boxes}")
    rgb = got[0][0, 1, :3]  # the grey frame comes back grey under every order (max == min: the hue leaves it alone)
    assert torch.equal(rgb[0], rgb[1]) and torch.equal(rgb[0], rgb[2])


def test_identity(dev):
    """The full box at the clip's size, no flip, no jitter: ``clip.unpack()`` bit for bit, and flow x zoom bit for bit
    where the flow has the clip's size."""
    from waldo_amd import functional as WF
    data, flow = clip_bytes(), make_flow((HD, WD))
    params = make_params((FULL, FULL), (0, 0), ((255,) * T,) * B)
    out, fl = run(dev, data, params, flow)
    assert torch.equal(out, WF.PackedClip(data.to(dev), NL).unpack())
    assert torch.equal(fl.cpu(), flow * torch.tensor(ZOOM).view(B, 1, 1, 1, 1))
    out2, none = run(dev, data, params)
    assert none is None and torch.equal(out2, out)


@pytest.mark.parametrize("out_size", [(20, 68), (23, 70)])
def test_crop_edges(dev, out_size):
    """A box == the same call on a clip that physically holds only that box: the taps clamp to the box, not to the
    image.  (The flow at the clip's size, cropped the same way: its first resize is the identity on both sides.)"""
    data, flow = clip_bytes(), make_flow((HD, WD))
    inner = (2, 3, 11, 29)  # not at an edge of the clip either
    for top, left, h, w in (CORNER, inner):
        params = make_params(((top, left, h, w),) * B, (0, 3))
        got = run(dev, data, params, flow, out_size)
        part = data[:, :, top:top + h, left:left + w].contiguous()
        part_flow = flow[..., top:top + h, left:left + w].contiguous()
        want = run(dev, part, make_params(((0, 0, h, w),) * B, (0, 3)), part_flow, out_size)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("out_size", [(20, 68), (23, 70)])
def test_flips(dev, out_size):
    """Left-right == ``.flip(-1)`` of the unflipped result with flow channel 0 negated; top-bottom likewise with
    ``.flip(-2)`` and channel 1; both together.  Bit for bit, jitter included."""
    data, flow = clip_bytes(), make_flow((8, 27))
    boxes = (CORNER, (3, 5, 13, 40))
    plain = run(dev, data, make_params(boxes, (0, 0)), flow, out_size)
    for bits in (1, 2, 3):
        got = run(dev, data, make_params(boxes, (bits, bits)), flow, out_size)
        dims = [d for d, bit in ((-1, 1), (-2, 2)) if bits & bit]
        sign = torch.tensor([-1.0 if bits & 1 else 1.0, -1.0 if bits & 2 else 1.0], device=dev).view(1, 1, 2, 1, 1)
        assert torch.equal(got[0], plain[0].flip(dims)), bits
        assert torch.equal(got[1], plain[1].flip(dims) * sign), bits


def test_two_stage_flow(dev):
    """An (8, 27) flow under a cropped box: the result is the composition of the reference's two bilinear resizes (to the
    clip's grid, then the crop's resize), which is not one bilinear sample at the composed position."""
    data, flow = clip_bytes(), make_flow((8, 27))
    out_size = (23, 70)
    params = make_params((CORNER, (3, 5, 13, 40)), (0, 0), zoom=(1.0, 1.0))
    got = run(dev, data, params, flow, out_size)
    compare(got, data, params, flow, out_size, "two-stage")
    single = torch.empty(B, T, 2, *out_size, dtype=torch.float64)
    for i in range(B):
        top, left, hc, wc = (int(v) for v in params.box[i])
        sy = ((torch.arange(out_size[0], dtype=torch.float64) + 0.5) * hc / out_size[0] - 0.5).clamp(0, hc - 1) + top
        sx = ((torch.arange(out_size[1], dtype=torch.float64) + 0.5) * wc / out_size[1] - 0.5).clamp(0, wc - 1) + left
        # (sy, sx) on the clip's grid -> normalised coordinates of the flow's own grid, one bilinear sample each
        gy = ((sy + 0.5) * 8 / HD - 0.5).clamp(0, 7) / 7 * 2 - 1
        gx = ((sx + 0.5) * 27 / WD - 0.5).clamp(0, 26) / 26 * 2 - 1
        grid = torch.stack(torch.broadcast_tensors(gx[None, :], gy[:, None]), dim=-1).expand(T, -1, -1, -1)
        single[i] = F.grid_sample(flow[i].double(), grid, mode="bilinear", align_corners=True)
    gap = (got[1].cpu().double() - single).abs().max().item()
    bound = TOL * flow.abs().max().item()
    print(f"[augment] two resizes against one sample: max gap {gap:.3e}, parity bound {bound:.3e}")
    assert gap > 10 * bound


def test_tables_are_clamped(dev):
    """Boxes mildly out of range on a clip and a flow that are the middle slice of buffers three clips long (an unclamped
    read would land inside the allocation and give a wrong value, not a fault): the result is that of the clamped boxes.
    An order byte of 9 is 255."""
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    data3, flow3 = clip_bytes(seed=4, b=3).to(dev), make_flow((8, 27), seed=5, b=3).to(dev)
    clip, flow = WF.PackedClip(data3[1:2], NL), flow3[1:2]

    def call(box, order):
        p = A.AugmentParams(torch.tensor([box], dtype=torch.int32), torch.tensor([1], dtype=torch.uint8),
                            torch.tensor([JITTER[0]]), torch.tensor([order], dtype=torch.uint8), torch.tensor([ZOOM[0]]))
        out = A.augment_clip(clip, p.to(dev), flow=flow, out_size=(23, 70))
        torch.cuda.synchronize()
        return p, out

    for wild, tame in (((-2, WD - 1, HD + 3, 9), (0, WD - 1, HD, 1)), ((HD + 5, -7, 4, WD + 1), (HD - 1, 0, 1, WD)),
                       ((3, 5, -1, 0), (3, 5, 1, 1))):
        p, got = call(wild, (9, 255, 4))
        _, want = call(tame, (255, 255, 4))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), wild
        assert R.clamped_box(wild, HD, WD) == tame
    compare(got, data3[1:2].cpu(), p, flow.cpu(), (23, 70), "clamped")


def test_one_launch_and_nothing_else(dev):
    """One call of the entry point per augment_clip, with or without a flow, and no framework op around it but the
    allocation of the results."""
    from waldo_amd import _lib
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    clip, flow = WF.PackedClip(clip_bytes().to(dev), NL), make_flow((8, 27)).to(dev)
    params = make_params((FULL, CORNER), (1, 2)).to(dev)
    for fl in (None, flow):
        with _lib.KernelTimer() as timer:
            A.augment_clip(clip, params, flow=fl, out_size=(23, 70))
        torch.cuda.synchronize()
        assert {k: v[0] for k, v in timer.summary().items()} == {"waldo_augment_clip_fwd": 1}
    torch.cuda.set_sync_debug_mode("error")  # (and no host synchronisation)
    try:
        A.augment_clip(clip, params, flow=flow, out_size=(23, 70))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        A.augment_clip(clip, params, flow=flow, out_size=(23, 70))
    ops = {e.key for e in prof.key_averages() if e.key.startswith("aten::")}
    assert ops <= {"aten::empty", "aten::detach"}, ops


def test_graph_capture_reads_the_tables_at_replay(dev):
    """augment_clip captured with device-resident tables (one kernel node: a single chain); the tables overwritten in
    place; the replay == an eager call with the new tables, bit for bit."""
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    clip, flow = WF.PackedClip(clip_bytes().to(dev), NL), make_flow((8, 27)).to(dev)
    params = make_params((FULL, CORNER), (0, 0), ((255,) * T,) * B).to(dev)
    out = torch.zeros(B, T, 3 + NL, 23, 70, device=dev)
    flow_out = torch.zeros(B, T, 2, 23, 70, device=dev)
    A.augment_clip(clip, params, flow=flow, out_size=(23, 70), out=out, flow_out=flow_out)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = A.augment_clip(clip, params, flow=flow, out_size=(23, 70), out=out, flow_out=flow_out)
    assert res[0] is out and res[1] is flow_out
    new = make_params(BOXES["pixel+odd"], (3, 1), ORDERS["b"], zoom=(0.5, 2.0)).to(dev)
    params.copy_(new)
    out.zero_()
    flow_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = A.augment_clip(clip, new, flow=flow, out_size=(23, 70))
    assert torch.equal(out, want[0]) and torch.equal(flow_out, want[1])
    assert not torch.equal(out, A.augment_clip(clip, make_params((FULL, CORNER), (0, 0)).to(dev), out_size=(23, 70))[0])


def test_augmenter(dev):
    """The same generator seed gives the same sample; sampled tables pass check_params; ``train=False`` is the crop and
    resize of min_zoom without jitter -- here the identity."""
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(11)
    data = torch.randint(0, 256, (4, T, 20, 40, 4), generator=g, dtype=torch.uint8)
    data[..., 3] %= NL
    clip = WF.PackedClip(data.to(dev), NL)
    flow = 0.1 * torch.randn(4, T, 2, 10, 20, generator=g).to(dev)
    aug = A.Augmenter(size=(24, 48), aspect_ratio=2.0, true_ratio=2.0, max_zoom=1.3, lr_flip=True, tb_flip=True,
                      colorjitter=0.5)
    first = aug(clip, flow=flow, generator=torch.Generator(device=dev).manual_seed(7))
    again = aug(clip, flow=flow, generator=torch.Generator(device=dev).manual_seed(7))
    other = aug(clip, flow=flow, generator=torch.Generator(device=dev).manual_seed(8))
    assert first[0].shape == (4, T, 3 + NL, 24, 48) and first[1].shape == (4, T, 2, 24, 48)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert not torch.equal(first[0], other[0])
    params = aug.params(clip, torch.Generator(device=dev).manual_seed(7))
    A.check_params(params, clip.shape)
    assert params.box.device == clip.device and (params.box[:, 2] <= 20).all() and (params.box[:, 2] >= 15).all()
    compare(first, data, params.to("cpu"), flow.cpu(), (24, 48), "augmenter")
    plain = A.Augmenter(aspect_ratio=2.0, true_ratio=2.0, max_zoom=1.3, lr_flip=True, tb_flip=True, colorjitter=0.5)
    out, fl = plain(clip, train=False)
    assert fl is None and torch.equal(out, clip.unpack())
    kitti = A.Augmenter(size=(20, 50), aspect_ratio=2.5, true_ratio=2.0, max_zoom=1.3, colorjitter=0.5)  # min_zoom 1.25
    p = kitti.params(clip, train=False)
    assert p.box.tolist() == [[0, 0, 16, 40]] * 4 and (p.order == 255).all() and (p.flip == 0).all()
    assert torch.equal(kitti(clip, train=False)[0], A.augment_clip(clip, p, out_size=(20, 50))[0])
