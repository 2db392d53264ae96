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
fails.

    python tools_dev/ab_unet.py --dtype bf16 [--out profiles/unet_16bit.json] [--sections op,unet]

``--dtype bf16|fp16``: the 16-bit form (``out_dtype`` / ``UNet.act_dtype``) under ``torch.autocast`` of that type, THREE
routes alternating: ``framework`` (a: ``fused = False`` under autocast), ``fp32_kernel`` (b: the fp32 kernel with
autocast's casts around it -- ``out_dtype=None``, the module without ``act_dtype`` inside an autocast region) and
``kernel16`` (c: the 16-bit kernel).  In the op section x, skip and grad_out are of the 16-bit type, as a convolution
under autocast hands them over, and routes (a) and (b) end with the cast to it that the NEXT convolution makes of their
fp32 result (their backward then starts with its widening): what route (c) replaces.  Results go under the dtype's name;
``c_slower_than_a`` / ``_b`` say median(c) > median(a | b) * (1 + spread).  The comparators are (a) and (b), never (c)
itself."""
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
    if "kernel16" in out:
        for tag, other in (("a", "framework"), ("b", "fp32_kernel")):
            out[f"c_over_{tag}"] = out["kernel16"]["median_ms"] / out[other]["median_ms"]
            out[f"c_slower_than_{tag}"] = bool(out["kernel16"]["median_ms"] > out[other]["median_ms"] * (1 + spread))
        return out
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


def kernel_route(*args, **kw):
    """WF.plane_norm_gelu with the launcher's gate open: the op section times the KERNEL at every shape (the gate is
    set from its numbers); the unet and predict sections run the module as it ships."""
    saved = WF.PLANE_NORM_GRAD_FRAMEWORK_HW, WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP
    WF.PLANE_NORM_GRAD_FRAMEWORK_HW = WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP = ()
    try:
        return WF.plane_norm_gelu(*args, **kw)
    finally:
        WF.PLANE_NORM_GRAD_FRAMEWORK_HW, WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP = saved


def routes16(dtype):
    """The three routes of the op under autocast of ``dtype`` (the module's docstring), name -> callable."""
    def under(fn):
        def call(*args):
            with torch.autocast("cuda", dtype=dtype):
                return fn(*args)
        return call
    return {"framework": under(lambda *a: WF.plane_norm_gelu_framework(*a).to(dtype)),
            "fp32_kernel": under(lambda *a: kernel_route(*a).to(dtype)),
            "kernel16": under(lambda *a: kernel_route(*a, out_dtype=dtype))}


def op_section(dev, images, warmup, rounds, save, dtype=None):
    res = {}
    first, store = ("kernel16", dtype) if dtype is not None else ("fused", torch.float32)
    for name, c, cs, h, w in level_shapes():
        g = torch.Generator().manual_seed(c + h)
        x = torch.randn(images, c, h, w, generator=g).to(dev, store)
        skip = torch.randn(images, cs, h, w, generator=g).to(dev, store) if cs else None
        weight, bias = (1 + 0.1 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
        go = torch.randn(images, c + cs, h, w, generator=g).to(dev, store)
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

        routes = {"fused": kernel_route, "framework": WF.plane_norm_gelu_framework} if dtype is None else routes16(dtype)
        with torch.no_grad():
            a, b = (routes[k](x, weight, bias, skip) for k in (first, "framework"))
            err = (a.float() - b.float()).abs().max().item()
        entry = dict(C=c, Cs=cs, H=h, W=w, images=images, max_abs_difference=err,
                     forward=alternate({k: (lambda fn=fn: fwd(fn)) for k, fn in routes.items()}, warmup, rounds),
                     forward_backward=alternate({k: (lambda fn=fn: fwd_bwd(fn)) for k, fn in routes.items()}, warmup, rounds),
                     peak_bytes_forward_backward={k: peak_above_inputs(lambda fn=fn: fwd_bwd(fn)) for k, fn in routes.items()})
        units = images * c * h * w * x.element_size()
        entry["x_bytes"] = units
        res[name] = entry
        if dtype is None:
            print(f"{name}: C {c} Cs {cs} {h}x{w}  fwd {entry['forward']['fused']['median_ms']:.3f} vs "
                  f"{entry['forward']['framework']['median_ms']:.3f} ms  fwd+bwd "
                  f"{entry['forward_backward']['fused']['median_ms']:.3f} vs "
                  f"{entry['forward_backward']['framework']['median_ms']:.3f} ms  slower: "
                  f"{entry['forward']['fused_slower']} / {entry['forward_backward']['fused_slower']}", flush=True)
        else:
            print(f"{name}: C {c} Cs {cs} {h}x{w}  " + "  ".join(
                f"{m} a/b/c " + "/".join(f"{entry[m][k]['median_ms']:.3f}" for k in routes) +
                f" ms spread {entry[m]['spread']:.3f} c slower than a/b: {entry[m]['c_slower_than_a']}/"
                f"{entry[m]['c_slower_than_b']}" for m in ("forward", "forward_backward")), flush=True)
        save("op", res)
        del x, skip, go, leaves, a, b
        torch.cuda.empty_cache()
    return res


def unet_section(dev, images, warmup, rounds, grad, save, key, dtype=None):
    torch.manual_seed(0)
    net = UNet(CIN, COUT, EMBED, "ln2d", DEPTH, 1, False, "bilinear").to(dev)
    x = torch.randn(images, CIN, H, W, device=dev)
    go = torch.randn(images, COUT, H, W, device=dev, dtype=dtype or torch.float32)

    def call(fused, backward, act_dtype=None):
        """``fused`` with ``dtype`` and no ``act_dtype``: the module as it was before the 16-bit form, inside an autocast
        region -- the fp32 kernel with casts around it."""
        net.fused, net.act_dtype = fused, act_dtype
        with torch.autocast("cuda", dtype=dtype or torch.bfloat16, enabled=dtype is not None):
            if not backward:
                with torch.no_grad():
                    return net(x)
            net.zero_grad(set_to_none=True)
            out = net(x)
        out.backward(go)
        return out

    if dtype is None:
        routes = {"fused": (True, None), "framework": (False, None)}
    else:
        routes = {"framework": (False, dtype), "fp32_kernel": (True, None), "kernel16": (True, dtype)}
    first = "fused" if dtype is None else "kernel16"
    res = dict(images=images, C=CIN, H=H, W=W, depth=DEPTH, embed_dim=EMBED)
    with torch.no_grad():
        res["max_abs_difference"] = (call(*routes[first][:1], False, routes[first][1]).float()
                                     - call(routes["framework"][0], False, routes["framework"][1]).float()).abs().max().item()
    modes = [("forward", False)] + ([("forward_backward", True)] if grad else [])
    for name, backward in modes:
        res[name] = alternate({k: (lambda f=f, a=a: call(f, backward, a)) for k, (f, a) in routes.items()}, warmup, rounds)
        res["peak_bytes_" + name] = {k: peak_above_inputs(lambda f=f, a=a: call(f, backward, a))
                                     for k, (f, a) in routes.items()}
        print(f"{key} {name}: " + ", ".join(f"{k} {res[name][k]['median_ms']:.2f} ms" for k in routes) +
              f", spread {res[name]['spread']:.3f}, peak {res['peak_bytes_' + name]}", flush=True)
        save(key, res)
    net.act_dtype = None
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="profiles/unet.json; with --dtype: profiles/unet_16bit.json")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default=None,
                    help="the 16-bit form under autocast: three routes (the module's docstring)")
    ap.add_argument("--sections", default="op,unet,predict")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--predict-images", type=int, default=160)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_unet: needs a GPU")
    dev = torch.device("cuda:0")
    dtype = {None: None, "bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "unet.json" if dtype is None else "unet_16bit.json")
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, limits=WF.plane_norm_limits(),
               gate=dict(grad_framework_hw=[list(r) for r in WF.PLANE_NORM_GRAD_FRAMEWORK_HW],
                         grad_framework_hw_no_skip=[list(r) for r in WF.PLANE_NORM_GRAD_FRAMEWORK_HW_NO_SKIP]), rounds=args.rounds, warmup=args.warmup)

    def save(key, value):
        (doc if dtype is None else doc.setdefault(args.dtype, {}))[key] = value
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)

    sections = args.sections.split(",")
    if "op" in sections:
        op_section(dev, args.images, args.warmup, args.rounds, save, dtype)
    if "unet" in sections:
        unet_section(dev, args.images, args.warmup, args.rounds, True, save, "unet", dtype)
    if "predict" in sections:
        unet_section(dev, args.predict_images, args.warmup, args.rounds, False, save, "predict", dtype)
    print(args.out)


if __name__ == "__main__":
    main()
