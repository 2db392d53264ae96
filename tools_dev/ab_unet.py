"""A/B of the fused plane norm (WF.plane_norm_gelu, csrc/plane_norm.hip) against the framework route (GroupNorm -> GELU ->
torch.cat) at the WIF recipe's shapes -- ``ii_depth 6``, ``ii_embed_dim 512``, 40 input channels, 512 x 1024 -- on one
MI355X.  Writes profiles/unet.json.

    python tools_dev/ab_unet.py [--out profiles/unet.json] [--sections op,unet,predict] [--images 8] [--rounds 20]

Sections:
  op       the op alone at each of the twelve level shapes (six encoder levels without a skip, six decoder levels with
           one), forward (no autograd) and forward + backward, --images images; the kernel with the launcher's gate
           open (``kernel_route``): the gate is set from these numbers;
  unet     the whole ``waldo_amd.modules.UNet``, ``fused`` True against False of the SAME module, forward and forward +
           backward at the training shape (--images x 40 x 512 x 1024);
  predict  its forward without autograd at one C5 predict's image count (--predict-images, 160).
Method: device time between events; the two routes ALTERNATE inside one process (fused, framework, fused, ...), --rounds
rounds after --warmup of each; median, minimum and quartiles per route.  ``spread`` is the larger of the two routes'
interquartile ranges over their medians; ``fused_slower`` says median(fused) > median(framework) * (1 + spread).  Peak
memory is ``max_memory_allocated`` above what was allocated before the call (the inputs and parameters), one call each.
Acceptance is relative to the framework route of the same run, never to the code under test alone.  A run without a GPU
fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from waldo_amd import functional as WF  # noqa: E402
from waldo_amd.modules import UNet  # noqa: E402

DEPTH, EMBED, CIN, COUT, H, W = 6, 512, 40, 5, 512, 1024


def level_shapes():
    """(name, C, Cs, h, w) of the twelve norm -> GELU (-> cat) sites, in the order the forward meets them."""
    base = EMBED // 2 ** (DEPTH - 1)
    enc = [(f"enc{i}", base * 2 ** (i + 1), 0, H >> (i + 1), W >> (i + 1)) for i in range(DEPTH)]
    dec = [(f"dec{i}", base * 2 ** i, base * 2 ** i, H >> i, W >> i) for i in reversed(range(DEPTH))]
    return enc + dec


def alternate(routes, warmup, rounds):
    """{name: stats} of callables timed alternately: one call of each per round."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ms.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        out[k] = dict(median_ms=med, min_ms=float(np.min(v)), q1_ms=q1, q3_ms=q3, rounds=len(v))
    spread = max((s["q3_ms"] - s["q1_ms"]) / s["median_ms"] for s in out.values())
    out["spread"] = spread
    out["fused_over_framework"] = out["fused"]["median_ms"] / out["framework"]["median_ms"]
    out["fused_slower"] = bool(out["fused"]["median_ms"] > out["framework"]["median_ms"] * (1 + spread))
    return out


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del keep
    return int(peak)


def kernel_route(*args):
    """WF.plane_norm_gelu with the launcher's gate open: the op section times the KERNEL at every shape (the gate is
    set from its numbers); the unet and predict sections run the module as it ships."""
    saved = WF.PLANE_NORM_GRAD_FRAMEWORK_HW, WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP
    WF.PLANE_NORM_GRAD_FRAMEWORK_HW = WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP = ()
    try:
        return WF.plane_norm_gelu(*args)
    finally:
        WF.PLANE_NORM_GRAD_FRAMEWORK_HW, WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP = saved


def op_section(dev, images, warmup, rounds, save):
    res = {}
    for name, c, cs, h, w in level_shapes():
        g = torch.Generator().manual_seed(c + h)
        x = torch.randn(images, c, h, w, generator=g).to(dev)
        skip = torch.randn(images, cs, h, w, generator=g).to(dev) if cs else None
        weight, bias = (1 + 0.1 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
        go = torch.randn(images, c + cs, h, w, generator=g).to(dev)
        leaves = [t.clone().requires_grad_() for t in (x, weight, bias)] + [None if skip is None else skip.clone().requires_grad_()]

        def fwd(fn):
            with torch.no_grad():
                return fn(x, weight, bias, skip)

        def fwd_bwd(fn):
            for t in leaves:
                if t is not None:
                    t.grad = None
            out = fn(*leaves)
            out.backward(go)
            return out

        routes = {"fused": kernel_route, "framework": WF.plane_norm_gelu_framework}
        with torch.no_grad():
            a, b = (fn(x, weight, bias, skip) for fn in routes.values())
            err = (a - b).abs().max().item()
        entry = dict(C=c, Cs=cs, H=h, W=w, images=images, max_abs_difference=err,
                     forward=alternate({k: (lambda fn=fn: fwd(fn)) for k, fn in routes.items()}, warmup, rounds),
                     forward_backward=alternate({k: (lambda fn=fn: fwd_bwd(fn)) for k, fn in routes.items()}, warmup, rounds),
                     peak_bytes_forward_backward={k: peak_above_inputs(lambda fn=fn: fwd_bwd(fn)) for k, fn in routes.items()})
        units = images * c * h * w * 4
        entry["x_bytes"] = units
        res[name] = entry
        print(f"{name}: C {c} Cs {cs} {h}x{w}  fwd {entry['forward']['fused']['median_ms']:.3f} vs "
              f"{entry['forward']['framework']['median_ms']:.3f} ms  fwd+bwd "
              f"{entry['forward_backward']['fused']['median_ms']:.3f} vs "
              f"{entry['forward_backward']['framework']['median_ms']:.3f} ms  slower: "
              f"{entry['forward']['fused_slower']} / {entry['forward_backward']['fused_slower']}", flush=True)
        save("op", res)
        del x, skip, go, leaves, a, b
        torch.cuda.empty_cache()
    return res


def unet_section(dev, images, warmup, rounds, grad, save, key):
    torch.manual_seed(0)
    net = UNet(CIN, COUT, EMBED, "ln2d", DEPTH, 1, False, "bilinear").to(dev)
    x = torch.randn(images, CIN, H, W, device=dev)
    go = torch.randn(images, COUT, H, W, device=dev)

    def call(fused, backward):
        net.fused = fused
        if not backward:
            with torch.no_grad():
                return net(x)
        net.zero_grad(set_to_none=True)
        out = net(x)
        out.backward(go)
        return out

    res = dict(images=images, C=CIN, H=H, W=W, depth=DEPTH, embed_dim=EMBED)
    with torch.no_grad():
        res["max_abs_difference"] = (call(True, False) - call(False, False)).abs().max().item()
    modes = [("forward", False)] + ([("forward_backward", True)] if grad else [])
    for name, backward in modes:
        res[name] = alternate({"fused": lambda: call(True, backward), "framework": lambda: call(False, backward)},
                              warmup, rounds)
        res["peak_bytes_" + name] = {k: peak_above_inputs(lambda f=f: call(f, backward))
                                     for k, f in (("fused", True), ("framework", False))}
        print(f"{key} {name}: fused {res[name]['fused']['median_ms']:.2f} ms, framework "
              f"{res[name]['framework']['median_ms']:.2f} ms, peak {res['peak_bytes_' + name]}", flush=True)
        save(key, res)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet.json"))
    ap.add_argument("--sections", default="op,unet,predict")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--predict-images", type=int, default=160)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_unet: needs a GPU")
    dev = torch.device("cuda:0")
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, limits=WF.plane_norm_limits(),
               gate=dict(grad_framework_hw=[list(r) for r in WF.PLANE_NORM_GRAD_FRAMEWORK_HW],
                         grad_framework_hw_no_skip=[list(r) for r in WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP]), rounds=args.rounds, warmup=args.warmup)

    def save(key, value):
        doc[key] = value
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)

    sections = args.sections.split(",")
    if "op" in sections:
        op_section(dev, args.images, args.warmup, args.rounds, save)
    if "unet" in sections:
        unet_section(dev, args.images, args.warmup, args.rounds, True, save, "unet")
    if "predict" in sections:
        unet_section(dev, args.predict_images, args.warmup, args.rounds, False, save, "predict")
    print(args.out)


if __name__ == "__main__":
    main()
