"""A/B of the renders (waldo_amd.render) at the Cityscapes recipe's shapes -- 56 frames of 512 x 1024, Nl = 20 layout
classes, L = 12 object layers, Tc = 4 contexts -- against the same results spelled in framework ops on the device and
against the reference's host route.  Writes profiles/render.json.

    python tools_dev/ab_render.py [--out profiles/render.json] [--frames 56] [--height 512] [--width 1024] [--lib PATH]

Routes, each producing the SAME bytes (checked here, at the timed size, before anything is timed):
  new        one library call: render_argmax(..., return_ids=True) / class_ids / render_flow;
  framework  x.max(dim)[1] -> palette index -> permute -> uint8 (the flow: the formula in torch ops), on the device --
             what a caller could write without this library's kernels;
  host       the reference's route (tools/logger.py:169-202, 265-318; tools/utils.py:202-214): .cpu(), max into
             int64, then per frame a colormap lookup in float64, (255 x).astype(uint8), PIL, byte / 255 and the
             normalisation -- restated with numpy / PIL (matplotlib's ListedColormap where it is installed).  Timed
             on --host-frames frames and scaled to the clip: it is linear in the frame count.
Times are device-event medians of --iters calls after --warmup (the alternation new / framework repeated in one process);
rates are the ALGORITHMIC bytes -- (4 C + 3) H W per frame for the palette render with fp32 planes ((4 C + 4) with the ids),
11 H W for the flow -- over the time, next to this box's copy rate measured here in the same run.
The flow render's share of bytes that differ from the reference's own (the fixture of tests/test_gpu_render.py) is
recorded too.  A run without a GPU fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from waldo_amd import _lib  # noqa: E402
from waldo_amd import render as R  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def framework_argmax(x, pal_dev):
    ids = x.max(dim=-3)[1]
    rgb = pal_dev[ids].movedim(-1, -3).contiguous()
    return rgb, ids.to(torch.uint8)


def framework_flow(flow, wheel_dev, mul=10.0):
    u, v = flow.select(-3, 0), flow.select(-3, 1)
    r = (u * u + v * v).sqrt() / float(np.float32(np.sqrt(2))) * mul
    r = torch.where(r > 1, torch.ones_like(r), r)
    theta = (1 + torch.atan2(v, u) / float(np.float32(np.pi))) / 2
    k = (theta * wheel_dev.shape[0]).long().clamp(0, wheel_dev.shape[0] - 1)
    rgb = (r.unsqueeze(-1) * wheel_dev[k]).clamp(0, 1) * 255.0
    return rgb.to(torch.uint8).movedim(-1, -3).contiguous()


def host_argmax(x, colormap):
    """The reference's get_lyt on ``x`` (frames, C, H, W): returns fp32 (frames, 3, H, W) in [-1, 1]."""
    import PIL.Image
    try:
        from matplotlib.colors import ListedColormap
        lookup = ListedColormap(colormap)
    except ImportError:
        lookup = lambda img: colormap[img]  # noqa: E731
    t = x.detach().cpu()
    ids = t.max(dim=-3)[1].numpy()
    out = torch.empty(ids.shape[0], 3, *ids.shape[-2:])
    for i in range(ids.shape[0]):
        rgba = lookup(ids[i].astype("uint8"))
        img = PIL.Image.fromarray((255 * np.delete(rgba, 3, 2)).astype("uint8"))
        ten = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)
        out[i] = (ten - 0.5) / 0.5
    return out


def host_flow(flow, wheel, mul=10.0):
    """The reference's get_flow_rgb on ``flow`` (frames, 2, H, W)."""
    f = flow.detach().cpu().permute(0, 2, 3, 1)
    r = (f ** 2).sum(-1).sqrt() / np.sqrt(2) * mul
    r[r > 1] = 1.
    theta = (1 + torch.atan2(f.select(-1, -1), f.select(-1, 0)) / np.pi) / 2
    k = np.minimum((theta.numpy() * wheel.shape[0]).astype(np.int64), wheel.shape[0] - 1)
    rgb = torch.tensor(wheel[k]).float()
    return (r.unsqueeze(-1) * rgb).permute(0, 3, 1, 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--frames", type=int, default=56)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--num-lyt", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--ctx", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--lib", default=None, help="another build of the library, timed under this script")
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    if not torch.cuda.is_available():
        raise SystemExit("ab_render: needs a GPU (no timing is taken without one)")
    dev = torch.device("cuda:0")
    n, h, w, nl, nlay = args.frames, args.height, args.width, args.num_lyt, args.layers
    hw = h * w
    g = torch.Generator(device=dev).manual_seed(0)
    output = torch.randn(1, n, 3 + nl, h, w, device=dev, generator=g)        # the decoded clip: rgb + layout channels
    lyt = output[:, :, 3:3 + nl]                                             # read in place
    alpha = torch.randn(1, n, nlay, h, w, device=dev, generator=g)
    flow = torch.randn(1, args.ctx, n // args.ctx, 2, h, w, device=dev, generator=g) * 0.05
    nflow = args.ctx * (n // args.ctx)
    pal, lpal, wheel = R.layer_palette(nl), R.layer_palette(nlay), R.flow_wheel()
    pal_dev, lpal_dev = torch.from_numpy(pal.copy()).to(dev), torch.from_numpy(lpal.copy()).to(dev)
    wheel_dev = torch.from_numpy(wheel).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(frames=n, H=h, W=w, Nl=nl, L=nlay, Tc=args.ctx),
           "timing": f"device events, median (min, max) of {args.iters} calls after {args.warmup}, best of "
                     f"{args.rounds} alternating rounds"}

    # the copy rate of this box, measured the way DESIGN section 0 does: a device-to-device copy, read + write bytes
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms, _, _ = timed(lambda: dst.copy_(src), 3, 10)
    copy_rate = 2 * src.numel() / (ms * 1e-3)
    res["copy_rate_TBps"] = copy_rate / 1e12
    del src, dst

    # the same bytes on every route, at the timed size
    rgb, ids = R.render_argmax(lyt, pal, return_ids=True)
    frgb, fids = framework_argmax(lyt, pal_dev)
    assert torch.equal(rgb, frgb) and torch.equal(ids, fids), "argmax routes differ"
    assert torch.equal(R.render_argmax(alpha, lpal), framework_argmax(alpha, lpal_dev)[0])
    pic, fpic = R.render_flow(flow), framework_flow(flow, wheel_dev)
    d = (pic.int() - fpic.int()).abs()
    res["flow_vs_framework"] = dict(differing_bytes_share=float((d != 0).float().mean()), max_levels=int(d.max()))
    del frgb, fids, fpic, d

    cases = {
        "sem_lyt_rgb_and_ids": (lambda: R.render_argmax(lyt, pal, return_ids=True), lambda: framework_argmax(lyt, pal_dev),
                                n * (4 * nl + 4) * hw),
        "sem_lyt_rgb": (lambda: R.render_argmax(lyt, pal), lambda: framework_argmax(lyt, pal_dev)[0], n * (4 * nl + 3) * hw),
        "class_ids": (lambda: R.class_ids(lyt), lambda: lyt.max(dim=-3)[1].to(torch.uint8), n * (4 * nl + 1) * hw),
        "obj_lyt_rgb": (lambda: R.render_argmax(alpha, lpal), lambda: framework_argmax(alpha, lpal_dev)[0],
                        n * (4 * nlay + 3) * hw),
        "flow_rgb": (lambda: R.render_flow(flow), lambda: framework_flow(flow, wheel_dev), nflow * 11 * hw),
    }
    for name, (new, fw, nbytes) in cases.items():
        best = {}
        for _ in range(args.rounds):  # alternate the two routes
            for route, fn in (("new", new), ("framework", fw)):
                t = timed(fn, args.warmup, args.iters)
                if route not in best or t[0] < best[route][0]:
                    best[route] = t
        res[name] = dict(
            algorithmic_bytes=nbytes,
            new_ms=best["new"][0], new_min_max_ms=best["new"][1:], framework_ms=best["framework"][0],
            framework_min_max_ms=best["framework"][1:], framework_over_new=best["framework"][0] / best["new"][0],
            new_TBps=nbytes / (best["new"][0] * 1e-3) / 1e12,
            new_share_of_copy_rate=nbytes / (best["new"][0] * 1e-3) / copy_rate)
        print(name, json.dumps(res[name]), flush=True)

    # the reference's host route, on a few frames, scaled to the clip
    k = min(args.host_frames, n)
    colormap = np.concatenate([R.colormap_table("jet", nl + 1)[(np.linspace(0, 1, nl + 1)[:nl] * (nl + 1)).astype(int)],
                               np.ones((nl, 1))], axis=1)
    colormap[0, :3] = 0.5
    t0 = time.perf_counter()
    href = host_argmax(lyt[0, :k], colormap)
    t_lyt = (time.perf_counter() - t0) * n / k
    back = torch.from_numpy(np.round((href.numpy().astype(np.float64) * 0.5 + 0.5) * 255).astype(np.uint8))
    assert torch.equal(back, rgb[0, :k].cpu()), "the host route's bytes differ"
    fl = flow.reshape(-1, 2, h, w)
    t0 = time.perf_counter()
    hflow = host_flow(fl[:k], wheel)
    t_flow = (time.perf_counter() - t0) * nflow / k
    hb = (hflow.clamp(0, 1) * 255.0).to(torch.uint8)
    d = (hb.int() - pic.reshape(-1, 3, h, w)[:k].cpu().int()).abs()
    res["host_route"] = dict(frames_timed=k, sem_lyt_ms_scaled_to_clip=t_lyt * 1e3, flow_ms_scaled_to_clip=t_flow * 1e3,
                             flow_differing_bytes_share=float((d != 0).float().mean()), flow_max_levels=int(d.max()))
    print("host_route", json.dumps(res["host_route"]), flush=True)

    # the flow render against the reference's own bytes (the fixture)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "render_reference.npz"))
    want = (torch.from_numpy(fx["flow_rgb"]).clamp(0, 1) * 255.0).to(torch.uint8)
    got = R.render_flow(torch.from_numpy(fx["flow"]).permute(0, 3, 1, 2).to(dev)).cpu()
    d = (got.int() - want.int()).abs()
    res["flow_vs_reference_fixture"] = dict(bytes=int(d.numel()), differing_bytes_share=float((d != 0).float().mean()),
                                            differing_pixels_share=float((d != 0).any(dim=1).float().mean()),
                                            max_levels=int(d.max()))
    print("flow_vs_reference_fixture", json.dumps(res["flow_vs_reference_fixture"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
