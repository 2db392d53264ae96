"""dev: the clip augmentation (waldo_amd.augment) at the two recipe shapes -- LVD (8 x 14 frames, 128 x 256, Nl = 20,
flow 128 x 256) and WIF (8 x 5 frames, 512 x 1024, Nl = 20, flow 128 x 256) -- against two other routes to the same
sample:

  framework  the same result in framework ops on the device: one-hot, F.interpolate and the jitter in tensor ops
             (tests/augment_ref.py's jitter), clip by clip with the boxes read on the host;
  host       the reference's route in PIL and torch on the host, frames spread over at most 16 threads (decoding not
             counted: the PIL images and class maps are made before the clock starts).

    python tools_dev/ab_augment.py [--out profiles/augment.json] [--variant NAME=LIB.so ...] [--no-host]

Per shape: milliseconds per sample (median of event-timed blocks; eager calls and the replay of one captured graph), the
bytes the sample needs from its shapes, and the GB/s reached.  ``--variant``: the kernel alone under another build of the
library (tools_dev/build_variant.py, e.g. -DWALDO_AUG_PX=1 or -DWALDO_AUG_LAUNCHES=2), each in child processes of their
own, taken in alternation with the product library's over two rounds.  Nothing is gated on any ratio."""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools_dev"))

import augment_ref as R  # noqa: E402
from waldo_amd import _lib  # noqa: E402

SHAPES = {"LVD": dict(b=8, t=14, size=(128, 256), flow=(128, 256), nl=20),
          "WIF": dict(b=8, t=5, size=(512, 1024), flow=(128, 256), nl=20)}
FIELDS = dict(aspect_ratio=2.0, true_ratio=2.0, max_zoom=1.3, lr_flip=True, tb_flip=False, colorjitter=0.5)
HOST_THREADS = 16


def sample_bytes(s):
    """What one sample reads and writes, from its shapes: the clip's words and the flow in, 3 + Nl + 2 fp32 planes out."""
    frames, (h, w), (hf, wf) = s["b"] * s["t"], s["size"], s["flow"]
    return {"read": frames * (4 * h * w + 8 * hf * wf), "written": frames * 4 * (3 + s["nl"] + 2) * h * w}


def inputs(s, dev, seed=0):
    from waldo_amd import augment as A
    from waldo_amd import functional as WF
    g = torch.Generator(device=dev).manual_seed(seed)
    b, t, (h, w), nl = s["b"], s["t"], s["size"], s["nl"]
    rgb = torch.randint(0, 256, (b, t, 3, h // 8, w // 8), generator=g, device=dev, dtype=torch.uint8)
    rgb = F.interpolate(rgb.flatten(0, 1).float(), scale_factor=8, mode="bilinear").round().byte().view(b, t, 3, h, w)
    cls = torch.randint(0, nl, (b, t, h // 16, w // 16), generator=g, device=dev)
    cls = cls.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)  # piecewise-constant class maps
    clip = WF.pack_clip(rgb, cls, nl)
    flow = 0.05 * torch.randn(b, t, 2, *s["flow"], generator=g, device=dev)
    params = A.sample_params(b, t, generator=g, device=dev, size=(h, w), **FIELDS)
    return clip, flow, params


def time_blocks(fn, repeats, inner):
    """Median and spread of ``repeats`` event-timed blocks of ``inner`` calls, in ms per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms.sort()
    return {"ms": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def eager_and_graph(fn, repeats, inner):
    res = {"eager": time_blocks(fn, repeats, inner)}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    res["graph"] = time_blocks(graph.replay, repeats, inner)
    return res


def with_rates(res, nbytes):
    total = nbytes["read"] + nbytes["written"]
    for r in res.values():
        r["GBps"] = round(total / r["ms"] / 1e6, 1)
    return res


def kernel_route(clip, flow, params, size):
    from waldo_amd import augment as A
    b, t, c = clip.shape[:3]
    out = torch.empty(b, t, c, *size, device=clip.device)
    flow_out = torch.empty(b, t, 2, *size, device=clip.device)
    return (lambda: A.augment_clip(clip, params, flow=flow, out_size=size, out=out, flow_out=flow_out)), out, flow_out


def framework_route(clip, flow, params, size):
    """The same sample in framework ops on the device.  The boxes, flips and orders come from a host copy of the tables
    (slicing needs them on the host); the jitter values and the zoom stay on the device."""
    host = {k: v.cpu() for k, v in params.tensors().items()}
    nl, data = clip.num_lyt, clip.data
    hd, wd = data.shape[2:4]
    # (made here: a host -> device copy cannot be captured into a graph)
    signs = [torch.tensor([-1.0 if int(f) & 1 else 1.0, -1.0 if int(f) & 2 else 1.0], device=data.device).view(1, 2, 1, 1)
             for f in host["flip"]]

    def fn():
        outs, flows = [], []
        for i in range(data.shape[0]):
            top, left, hc, wc = (int(v) for v in host["box"][i])
            dims = [d for d, bit in ((-1, 1), (-2, 2)) if int(host["flip"][i]) & bit]
            crop = data[i, :, top:top + hc, left:left + wc]
            rgb = F.interpolate(crop[..., :3].permute(0, 3, 1, 2).float() / 255.0, size=size, mode="bilinear",
                                align_corners=False)
            lyt = F.interpolate(F.one_hot(crop[..., 3].long(), 256)[..., :nl].permute(0, 3, 1, 2).float(), size=size,
                                mode="bilinear", align_corners=False)
            fl = flow[i] if flow.shape[-2:] == (hd, wd) else F.interpolate(flow[i], size=(hd, wd), mode="bilinear",
                                                                           align_corners=False)
            fl = F.interpolate(fl[..., top:top + hc, left:left + wc], size=size, mode="bilinear",
                               align_corners=False) * params.zoom[i]
            if dims:
                rgb, lyt, fl = rgb.flip(dims), lyt.flip(dims), fl.flip(dims) * signs[i]
            rgb = torch.stack([R.jitter_frame(rgb[j], host["order"][i, j], params.jitter[i]) for j in range(rgb.shape[0])])
            outs.append(torch.cat([(rgb - 0.5) / 0.5, 5.0 * (2.0 * lyt - 1.0)], dim=1))
            flows.append(fl)
        return torch.stack(outs), torch.stack(flows)

    return fn


def host_route(clip, flow, params, size):
    """The reference's route on the host: PIL for the frames (make_augment_golden.pil_route), torch for the one-hot
    layout and the flow; one task per frame on at most HOST_THREADS threads, one torch thread each."""
    from PIL import Image
    from make_augment_golden import pil_route
    host = {k: v.cpu() for k, v in params.tensors().items()}
    data, flow_h = clip.data.cpu(), flow.cpu()
    b, t, hd, wd, _ = data.shape
    nl = clip.num_lyt
    images = [[Image.fromarray(data[i, j, :, :, :3].numpy()) for j in range(t)] for i in range(b)]
    classes = [[data[i, j, :, :, 3].long() for j in range(t)] for i in range(b)]
    out = torch.empty(b, t, 3 + nl, *size)
    flow_out = torch.empty(b, t, 2, *size)

    def frame(ij):
        i, j = divmod(ij, t)
        box, flip = host["box"][i].tolist(), int(host["flip"][i])
        top, left, hc, wc = box
        dims = [d for d, bit in ((-1, 1), (-2, 2)) if flip & bit]
        rgb = pil_route(images[i][j], box, flip, host["jitter"][i].tolist(), int(host["order"][i, j]), size)
        out[i, j, :3] = (torch.from_numpy(rgb.copy()).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5
        onehot = torch.zeros(nl, hd, wd).scatter_(0, classes[i][j][None], 1)
        lyt = F.interpolate(onehot[None, :, top:top + hc, left:left + wc], size=size, mode="bilinear",
                            align_corners=False)[0]
        fl = flow_h[i, j] * float(host["zoom"][i])
        if flip & 1:
            fl[0] = -fl[0]
        if flip & 2:
            fl[1] = -fl[1]
        fl = F.interpolate(fl[None], size=(hd, wd), mode="bilinear", align_corners=False)
        fl = F.interpolate(fl[..., top:top + hc, left:left + wc], size=size, mode="bilinear", align_corners=False)[0]
        out[i, j, 3:] = 5 * ((lyt.flip(dims) if dims else lyt) * 2 - 1)
        flow_out[i, j] = fl.flip(dims) if dims else fl

    def fn():
        with ThreadPoolExecutor(max_workers=min(HOST_THREADS, b * t)) as pool:
            list(pool.map(frame, range(b * t)))
        return out, flow_out

    return fn


def measure(args, kernel_only):
    dev = torch.device("cuda:0")
    doc = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, s in SHAPES.items():
        clip, flow, params = inputs(s, dev)
        nbytes = sample_bytes(s)
        entry = {"shape": {k: list(v) if isinstance(v, tuple) else v for k, v in s.items()}, "bytes": nbytes}
        fn, out, flow_out = kernel_route(clip, flow, params, s["size"])
        inner = 20 if name == "LVD" else 10
        entry["kernel"] = with_rates(eager_and_graph(fn, args.repeats, inner), nbytes)
        if not kernel_only:
            chain = framework_route(clip, flow, params, s["size"])
            ref = chain()
            torch.cuda.synchronize()
            entry["framework_max_abs_diff"] = {"out": float((ref[0] - out).abs().max()),
                                               "flow": float((ref[1] - flow_out).abs().max())}
            del ref
            entry["framework"] = with_rates(eager_and_graph(chain, max(3, args.repeats // 4), 2), nbytes)
            if not args.no_host:
                torch.set_num_threads(1)
                host = host_route(clip, flow, params, s["size"])
                got = host()
                entry["host_max_abs_diff_rgb"] = float((got[0][:, :, :3] - out.cpu()[:, :, :3]).abs().max())
                entry["host_max_abs_diff_layout_flow"] = [float((got[0][:, :, 3:] - out.cpu()[:, :, 3:]).abs().max()),
                                                          float((got[1] - flow_out.cpu()).abs().max())]
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    host()
                    ms.append((time.perf_counter() - t0) * 1e3)
                entry["host"] = {"ms": round(sorted(ms)[1], 2), "min": round(min(ms), 2), "max": round(max(ms), 2),
                                 "threads": min(HOST_THREADS, s["b"] * s["t"])}
        doc["shapes"][name] = entry
        del clip, flow, params, out, flow_out
        torch.cuda.empty_cache()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--variant", action="append", default=[], help="NAME=LIB.so: the kernel alone under another build")
    ap.add_argument("--kernel-only", action="store_true", help="(the child of --variant) the kernel alone; one JSON line")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    if args.kernel_only:
        print("AB_AUGMENT " + json.dumps(measure(args, True)), flush=True)
        return
    doc = measure(args, False)
    if args.variant:
        libs = [("product", None)] + [tuple(v.split("=", 1)) for v in args.variant]
        rounds = {name: [] for name, _ in libs}
        for r in range(2):
            for name, path in (libs if r == 0 else libs[::-1]):
                cmd = [sys.executable, os.path.abspath(__file__), "--kernel-only", "--repeats", str(args.repeats)]
                if path:
                    cmd += ["--lib", path]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
                if p.returncode != 0:  # (a failed child ends the session: nothing more is started on the device)
                    raise SystemExit(f"variant {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB_AUGMENT ")][-1]
                rounds[name].append({k: v["kernel"] for k, v in json.loads(line[len("AB_AUGMENT "):])["shapes"].items()})
        doc["kernel_variants"] = rounds
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
