"""dev: ``WIF.inpaint`` on a batch of four clips at the Cityscapes recipe's raster (512 x 1024, 12 layers, Tc = 4, Tp = 10,
the default option set, stub inpainter; inputs generated on the device) -- ONE batched call, with the one host read of
the border-object table and without any (``always_inpaint_borders``), against the only way there was before the border
objects were chosen on the device: four B = 1 calls in a loop.  Same process, the three variants interleaved, wall
time around a call that ends in a synchronise, median of 7 after 3 warm-ups.  One JSON document.

    python tools_dev/ab_inpaint_batch.py [--out profiles/inpaint_batch.json] [--clips 4] [--tp 10]"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from waldo_amd import _lib  # noqa: E402
from waldo_amd.nets import WIF, Warper  # noqa: E402
from waldo_amd.tools.utils import get_grid  # noqa: E402

HD, WD, CTX_LEN, NO, NL = 512, 1024, 4, 11, 20
KINDS = ("left", "both", "none", "left")  # which borders an object enters through, clip by clip


def stub_inpainter(img, mask, exp=True, is_masked=True):
    """A deterministic stand-in for the external inpainter: the hole filled with a smooth function of the visible part,
    clip by clip."""
    vis = (img * (1 - mask)).sum(dim=(2, 3), keepdim=True) / (1 - mask).sum(dim=(2, 3), keepdim=True).clamp_min(1.0)
    ramp = torch.linspace(-0.2, 0.2, img.shape[-1], device=img.device).view(1, 1, 1, -1)
    return img * (1 - mask) + mask * (vis + ramp)


def options():
    opt = types.SimpleNamespace(
        ii_score=True, ii_ab=True, use_inpainter=True, ii_last_only=False, fix_thresh=True, use_expansion=True,
        num_expansion=2, loop_ii=True, inpaint_obj=True, propagate_unique=True, use_shadows=True, soft_shadow=False,
        fix_mask=False, propagate_obj=True,
        latent_shape=[8, 16], obj_shape=[4, 4], time_dropout=False, num_obj=NO, patch_size=16, scale_factor=1, dim=128,
        aspect_ratio=2, load_dim=512, num_perm_grid=1, normalize_alpha=False, use_lyt_filtering=False,
        use_lyt_opacity=False, weight_cls=False, min_cls=0.0, include_self=False, no_filter=False, allow_ghost=False)
    return opt


def make_inputs(dev, clips, tp, seed=31):
    """Smooth frames, blobby alphas, objects that touch a border and move out: the structure of the inputs
    tests/test_inpaint.py times the one-clip call on, for `clips` clips."""
    g = torch.Generator(device=dev).manual_seed(seed)
    t, nlay = CTX_LEN + tp, NO + 1
    c = 3 + NL + nlay

    def smooth(*shape, lo=32):
        x = torch.randn(*shape[:-2], shape[-2] // lo, shape[-1] // lo, generator=g, device=dev)
        y = torch.nn.functional.interpolate(x.reshape(-1, 1, *x.shape[-2:]), size=shape[-2:], mode="bilinear")
        return y.reshape(*shape)

    b = clips
    d = dict(obj_pose=get_grid(4, 4).to(dev).view(1, 1, 1, 16, 2) * 0.4
             + 0.08 * torch.randn(b, t, NO, 16, 2, generator=g, device=dev),
             bg_pose=get_grid(8, 16).to(dev).view(1, 1, 1, 128, 2) + 0.01 * torch.randn(b, t, 1, 128, 2, generator=g, device=dev))
    # raw_output as decode_output hands it over: a (B, Tc, Tp, ...) view of the (B, Tp, Tc, ...) buffer the frame warp writes
    d["raw_output"] = smooth(b, tp, CTX_LEN, c, HD, WD).permute(0, 2, 1, 3, 4, 5)
    d["real_vid"] = smooth(b, t, 3, HD, WD).clamp(-1, 1)
    alpha = (2.5 * smooth(b, CTX_LEN, nlay, HD, WD)).tanh()
    alpha[:, :, 0] = alpha[:, :, 0] * 0.3 + 0.7
    d["alpha"] = alpha
    actx = (2.5 * smooth(b, CTX_LEN, tp, nlay, HD, WD)).tanh() * 0.5 - 0.45
    actx[:, :, :, 0] = (2.0 * smooth(b, CTX_LEN, tp, HD, WD) + 0.5).tanh()
    flow = 0.05 * smooth(b, CTX_LEN, tp, 2, HD, WD)
    for i in range(b):
        kind = KINDS[i % len(KINDS)]
        if kind in ("left", "both"):
            actx[i, :, -1, 1 + i % NO, 128:320, 0:80] = 0.95
            flow[i, -1, -1, 0, 128:320, 0:80] = -0.1
        if kind == "both":
            actx[i, :, -1, 3, 200:420, WD - 80:WD] = 0.95
            flow[i, -1, -1, 0, 200:420, WD - 80:WD] = 0.1
    d["alpha_ctx"], d["pred_flow"] = actx, flow
    gw = torch.Generator().manual_seed(seed + 1)
    d["weight"], d["bias"] = torch.randn(5, c, 1, 1, generator=gw) * 0.3, torch.randn(5, generator=gw) * 0.1
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "inpaint_batch.json"))
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--tp", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt = options()
    d = make_inputs(dev, args.clips, args.tp)
    lin = torch.nn.Conv2d(d["weight"].shape[1], 5, 1)
    with torch.no_grad():
        lin.weight.copy_(d["weight"])
        lin.bias.copy_(d["bias"])
    wif, warper = WIF(opt, unet=lin).to(dev), Warper(opt).to(dev)
    keys = ("raw_output", "alpha", "alpha_ctx", "real_vid", "pred_flow")
    with torch.no_grad():
        grid = warper(d["obj_pose"], d["bg_pose"])

    def call(sel):
        return wif.inpaint(stub_inpainter, *(d[k][sel] for k in keys), CTX_LEN, warper, [x[sel] for x in grid])

    def loop():
        wif.always_inpaint_borders = False
        return torch.cat([call(slice(i, i + 1)) for i in range(args.clips)])

    def batched():
        wif.always_inpaint_borders = False
        return call(slice(None))

    def batched_no_read():
        wif.always_inpaint_borders = True
        return call(slice(None))

    variants = {"loop_of_one_clip_calls": loop, "batched": batched, "batched_always_inpaint_borders": batched_no_read}
    times = {n: [] for n in variants}
    outs = {}
    with torch.no_grad():
        for r in range(args.warmup + args.repeats):
            for n, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[n].append((time.perf_counter() - t0) * 1e3)
                outs[n] = out
        sections = {}
        for n, fn in variants.items():  # the border-object section alone (device time between events), one more call each
            spans, inner = [], wif._border_objects

            def timed(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = inner(*a, **kw)
                e1.record()
                spans.append((e0, e1))
                return res

            wif._border_objects = timed
            try:
                with _lib.KernelTimer() as kt:
                    fn()
                    torch.cuda.synchronize()
            finally:
                del wif._border_objects
            sections[n] = {"border_objects_ms": round(sum(a.elapsed_time(b) for a, b in spans), 3),
                           "library_calls": sum(v[0] for v in kt.summary().values()),
                           "ms_in_library_calls": round(sum(v[0] * v[1] for v in kt.summary().values()), 3)}
    wif.always_inpaint_borders = False
    # (the stub's per-clip mean is a framework reduction: its summation order may depend on the batch size, so the frames
    # of the batched call may differ from the loop's in the last bits; tests/test_gpu_inpaint_batch.py compares with an
    # inpainter that is the same function of a clip whatever the batch)
    same = {n: float((outs[n] - outs["loop_of_one_clip_calls"]).abs().max()) for n in variants}
    doc = {"what": f"WIF.inpaint at {HD}x{WD}, B={args.clips}, Tc={CTX_LEN}, Tp={args.tp}, {NO + 1} layers, default option set "
                   f"(loop_ii, shadows, propagate_obj), stub inpainter; border objects per clip: {list(KINDS[:args.clips])}",
           "how": f"wall ms per call (ends in a synchronise), the variants interleaved in one process, median of "
                  f"{args.repeats} after {args.warmup} warm-ups",
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for n in variants:
        ts = sorted(times[n])
        doc["variants"][n] = {"ms_median": round(ts[len(ts) // 2], 3), "ms_best": round(ts[0], 3), "ms_worst": round(ts[-1], 3),
                              "ms_per_clip": round(ts[len(ts) // 2] / args.clips, 3),
                              "max_abs_difference_to_the_loop": same[n], **sections[n]}
    text = json.dumps(doc, indent=1)
    print(text)
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
