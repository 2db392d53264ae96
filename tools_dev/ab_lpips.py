"""A/B of the LPIPS level kernel (``WF.lpips_level``, include/waldo_hip.h "LPIPS level distance") against the chain of
framework ops it replaces (``WF.lpips_level_framework``), of the ``LPIPS`` module with either, and of the WIF training
step with and without the recipe's ``lpips_vid`` term, on one MI355X.  Writes profiles/lpips.json.

    python tools_dev/ab_lpips.py [--out profiles/lpips.json] [--rounds 20] [--warmup 3] [--sections level,module,step,alex]
                                 [--dtype bf16|fp16]

Sections:
  level   the op alone at VGG's five tap shapes -- 512 x 1024 frames with N = 2 (the WIF recipe: two clips x one
          predicted frame per GPU) and N = 8, 128 x 256 frames with N = 8: forward, and forward + backward to ``f0``;
          per shape the bytes the algorithm has to move (both maps read once; forward + backward: read twice, one
          gradient map written) and the rate that makes of the kernel's time.  ``gate`` applies the rule: the kernel
          unless the chain is faster by more than the spread both ways.
  module  ``LPIPS("vgg")`` forward + backward to ``in0`` on 2 frames of 512 x 1024, fused against ``fused=False``; the
          backbone alone (the same convolutions, the taps summed) for its share of the time; peak memory above the inputs.
  step    ``WifStep(2, objective="recipe", unet="reference")`` against ``objective="sharp"``.
  alex    ``LPIPS("alex")`` forward under no_grad on 40 frames of 512 x 1024 (one evaluation batch's predicted frames).
``--dtype bf16|fp16`` runs the 16-bit forms of the four sections instead and writes profiles/lpips_16bit.json (medians
of 15):
  level   taps stored in 16 bits, N = 2 and N = 8 frames of 512 x 1024: the 16-bit kernel (waldo_lpips_level_fwd_dt /
          _bwd_dt) against the chain on the widened taps and against the fp32 kernel on fp32 taps; the same gate rule,
          and ``faster_than_kernel32``: whether half the map bytes show beyond the spread.
  module  ``LPIPS("vgg", act_dtype=T)`` against ``fused=False`` under the same autocast and against the fp32 module.
  step    ``WifStep(2, objective="recipe", unet="reference", lpips_dtype=T)`` against the same step without it.
  alex    ``LPIPS("alex", act_dtype=T)`` forward on 40 frames against ``fused=False`` and the fp32 module.
Method: tools_dev/ab_lvd_nets.py's -- device time between events, the routes ALTERNATE inside one process, median /
minimum / quartiles per route, ``spread`` the largest interquartile range over its median.  Random weights (the
timings do not depend on them).  A run without a GPU fails."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ab_lvd_nets import alternate, peak_above_inputs  # noqa: E402
from waldo_amd import functional as WF  # noqa: E402
from waldo_amd.nets import LPIPS  # noqa: E402
from waldo_amd.nets.lpips import TAP_WIDTHS  # noqa: E402


def vgg_taps(n, h, w):
    return [(n, c, h >> k, w >> k) for k, c in enumerate(TAP_WIDTHS["vgg"])]


def level_section(dev, rounds, warmup):
    out = []
    for n, h, w in ((2, 512, 1024), (8, 512, 1024), (8, 128, 256)):
        for shape in vgg_taps(n, h, w):
            g = torch.Generator(device=dev).manual_seed(sum(shape))
            f0 = torch.randn(*shape, generator=g, device=dev).abs_().requires_grad_()
            f1 = torch.randn(*shape, generator=g, device=dev).abs_()
            wt = torch.rand(shape[1], generator=g, device=dev) * (2.0 / shape[1])
            grad_out = torch.ones(n, device=dev)
            routes = {"kernel": WF.lpips_level, "chain": WF.lpips_level_framework}

            def fwd(fn):
                with torch.no_grad():
                    return fn(f0, f1, wt)

            def fwd_bwd(fn):
                return torch.autograd.grad(fn(f0, f1, wt), f0, grad_out)

            row = dict(shape=list(shape), map_bytes=4 * f0.numel(),
                       fwd=alternate({k: (lambda fn=fn: fwd(fn)) for k, fn in routes.items()}, warmup, rounds),
                       fwd_bwd=alternate({k: (lambda fn=fn: fwd_bwd(fn)) for k, fn in routes.items()}, warmup, rounds))
            row["peak_bytes_fwd_bwd"] = {k: peak_above_inputs(lambda fn=fn: fwd_bwd(fn)) for k, fn in routes.items()}
            # algorithmic bytes: forward reads both maps; forward + backward reads them twice and writes one map
            row["fwd"]["kernel_algorithmic_gb_s"] = 2 * row["map_bytes"] / row["fwd"]["kernel"]["median_ms"] / 1e6
            row["fwd_bwd"]["kernel_algorithmic_gb_s"] = 5 * row["map_bytes"] / row["fwd_bwd"]["kernel"]["median_ms"] / 1e6
            slower = [s["kernel"]["median_ms"] * (1.0 - s["spread"]) > s["chain"]["median_ms"]
                      for s in (row["fwd"], row["fwd_bwd"])]
            row["gate"] = "chain" if all(slower) else "kernel"
            out.append(row)
            print(f"level {shape}: fwd kernel {row['fwd']['kernel']['median_ms']:.3f} chain {row['fwd']['chain']['median_ms']:.3f} ms; "
                  f"fwd+bwd kernel {row['fwd_bwd']['kernel']['median_ms']:.3f} chain {row['fwd_bwd']['chain']['median_ms']:.3f} ms; "
                  f"gate {row['gate']}", flush=True)
            del f0, f1
            torch.cuda.empty_cache()
    return out


def module_section(dev, rounds, warmup):
    torch.manual_seed(0)
    fused = LPIPS("vgg").to(dev)
    plain = LPIPS.load("vgg", state=fused.state_dict(), fused=False).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    in0 = (torch.rand(2, 3, 512, 1024, generator=g, device=dev) * 2 - 1).requires_grad_()
    in1 = torch.rand(2, 3, 512, 1024, generator=g, device=dev) * 2 - 1

    def run(m):
        return torch.autograd.grad(m(in0, in1).sum(), in0)

    def backbone():  # the same convolutions on both images, the taps of in0 summed in place of the levels
        a, b = fused.scaling_layer(in0), fused.scaling_layer(in1)
        total = 0
        for k in range(5):
            piece = getattr(fused.net, f"slice{k + 1}")
            a, b = piece(a), piece(b)
            total = total + a.sum()
        return torch.autograd.grad(total, in0)

    routes = {"fused": lambda: run(fused), "framework": lambda: run(plain), "backbone": backbone}
    sec = alternate(routes, warmup, rounds)
    sec["peak_bytes"] = {k: peak_above_inputs(fn) for k, fn in routes.items()}
    sec["shape"] = [2, 3, 512, 1024]
    for k in ("fused", "framework"):
        sec[k]["backbone_share"] = sec["backbone"]["median_ms"] / sec[k]["median_ms"]
    print(f"module vgg fwd+bwd: fused {sec['fused']['median_ms']:.2f} framework {sec['framework']['median_ms']:.2f} "
          f"backbone {sec['backbone']['median_ms']:.2f} ms", flush=True)
    return sec


def step_section(dev, rounds, warmup):
    from waldo_amd.tools.wif_step import WifStep
    steps = {k: WifStep(2, dev, objective=k, unet="reference") for k in ("recipe", "sharp")}
    sec = alternate({k: (lambda s=s: s()) for k, s in steps.items()}, warmup, rounds)
    sec["peak_bytes"] = {k: peak_above_inputs(lambda s=s: s()) for k, s in steps.items()}
    sec["terms"] = {k: float(v) for k, v in steps["recipe"].terms.items()}
    print(f"step: recipe {sec['recipe']['median_ms']:.2f} sharp {sec['sharp']['median_ms']:.2f} ms", flush=True)
    return sec


def alex_section(dev, rounds, warmup):
    torch.manual_seed(0)
    m = LPIPS("alex").to(dev)
    plain = LPIPS.load("alex", state=m.state_dict(), fused=False).to(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    in0 = torch.rand(40, 3, 512, 1024, generator=g, device=dev) * 2 - 1
    in1 = torch.rand(40, 3, 512, 1024, generator=g, device=dev) * 2 - 1

    def run(mod):
        with torch.no_grad():
            return mod(in0, in1)

    sec = alternate({"fused": lambda: run(m), "framework": lambda: run(plain)}, warmup, rounds)
    sec["frames"], sec["chunk"] = 40, m.chunk
    print(f"alex 40 frames fwd: fused {sec['fused']['median_ms']:.2f} framework {sec['framework']['median_ms']:.2f} ms",
          flush=True)
    return sec


DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def level16_section(dev, rounds, warmup, T):
    """The op at VGG's five taps of 2 and of 8 frames of 512 x 1024 on taps stored in T: the 16-bit kernel, the chain
    on the widened taps (what ``fused=False`` runs: the widening is part of its time) and the fp32 kernel on fp32 taps of
    the same values (what the fp32 module runs: twice the map bytes)."""
    out = []
    for n, h, w in ((2, 512, 1024), (8, 512, 1024)):
        for shape in vgg_taps(n, h, w):
            g = torch.Generator(device=dev).manual_seed(sum(shape))
            f0 = torch.randn(*shape, generator=g, device=dev).abs_().to(T).requires_grad_()
            f1 = torch.randn(*shape, generator=g, device=dev).abs_().to(T)
            x0, x1 = f0.detach().float().requires_grad_(), f1.float()
            wt = torch.rand(shape[1], generator=g, device=dev) * (2.0 / shape[1])
            grad_out = torch.ones(n, device=dev)
            routes = {"kernel16": lambda a, b: WF.lpips_level(a, b, wt),
                      "chain_widened": lambda a, b: WF.lpips_level_framework(a.float(), b.float(), wt),
                      "kernel32": lambda a, b: WF.lpips_level(x0, x1, wt)}
            leaf = {"kernel16": f0, "chain_widened": f0, "kernel32": x0}

            def fwd(k):
                with torch.no_grad():
                    return routes[k](f0, f1)

            def fwd_bwd(k):
                return torch.autograd.grad(routes[k](f0, f1), leaf[k], grad_out)

            row = dict(shape=list(shape), map_bytes=2 * f0.numel(), map_bytes_fp32=4 * f0.numel(),
                       fwd=alternate({k: (lambda k=k: fwd(k)) for k in routes}, warmup, rounds),
                       fwd_bwd=alternate({k: (lambda k=k: fwd_bwd(k)) for k in routes}, warmup, rounds))
            row["peak_bytes_fwd_bwd"] = {k: peak_above_inputs(lambda k=k: fwd_bwd(k)) for k in routes}
            # algorithmic bytes as in the fp32 section: forward reads both maps; forward + backward reads them twice
            # and writes one map
            row["fwd"]["kernel16_algorithmic_gb_s"] = 2 * row["map_bytes"] / row["fwd"]["kernel16"]["median_ms"] / 1e6
            row["fwd_bwd"]["kernel16_algorithmic_gb_s"] = 5 * row["map_bytes"] / row["fwd_bwd"]["kernel16"]["median_ms"] / 1e6
            slower = [s["kernel16"]["median_ms"] * (1.0 - s["spread"]) > s["chain_widened"]["median_ms"]
                      for s in (row["fwd"], row["fwd_bwd"])]
            row["gate"] = "chain" if all(slower) else "kernel"
            # the 16-bit kernel reads half the fp32 kernel's map bytes: faster beyond the spread, or a finding
            row["faster_than_kernel32"] = {
                name: bool(s["kernel16"]["median_ms"] < s["kernel32"]["median_ms"] * (1.0 - s["spread"]))
                for name, s in (("fwd", row["fwd"]), ("fwd_bwd", row["fwd_bwd"]))}
            out.append(row)
            print(f"level16 {shape}: fwd k16 {row['fwd']['kernel16']['median_ms']:.3f} chain {row['fwd']['chain_widened']['median_ms']:.3f} "
                  f"k32 {row['fwd']['kernel32']['median_ms']:.3f} ms (spread {row['fwd']['spread']:.3f}); fwd+bwd k16 "
                  f"{row['fwd_bwd']['kernel16']['median_ms']:.3f} chain {row['fwd_bwd']['chain_widened']['median_ms']:.3f} "
                  f"k32 {row['fwd_bwd']['kernel32']['median_ms']:.3f} ms (spread {row['fwd_bwd']['spread']:.3f}); "
                  f"gate {row['gate']}", flush=True)
            del f0, f1, x0, x1
            torch.cuda.empty_cache()
    return out


def module16_section(dev, rounds, warmup, T):
    """``LPIPS("vgg", act_dtype=T)`` forward + backward on 2 frames of 512 x 1024 against the fp32 module and against
    ``fused=False`` under the same autocast, in one process; peak memory above the inputs."""
    torch.manual_seed(0)
    fp32 = LPIPS("vgg").to(dev)
    fused = LPIPS.load("vgg", state=fp32.state_dict(), act_dtype=T).to(dev)
    plain = LPIPS.load("vgg", state=fp32.state_dict(), fused=False, act_dtype=T).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    in0 = (torch.rand(2, 3, 512, 1024, generator=g, device=dev) * 2 - 1).requires_grad_()
    in1 = torch.rand(2, 3, 512, 1024, generator=g, device=dev) * 2 - 1

    def run(m):
        return torch.autograd.grad(m(in0, in1).sum(), in0)

    routes = {"fused16": lambda: run(fused), "framework16": lambda: run(plain), "fp32": lambda: run(fp32)}
    sec = alternate(routes, warmup, rounds)
    sec["peak_bytes"] = {k: peak_above_inputs(fn) for k, fn in routes.items()}
    sec["shape"] = [2, 3, 512, 1024]
    print(f"module16 vgg fwd+bwd: fused16 {sec['fused16']['median_ms']:.2f} framework16 {sec['framework16']['median_ms']:.2f} "
          f"fp32 {sec['fp32']['median_ms']:.2f} ms (spread {sec['spread']:.3f})", flush=True)
    return sec


def step16_section(dev, rounds, warmup, T):
    from waldo_amd.tools.wif_step import WifStep
    steps = {"recipe16": WifStep(2, dev, objective="recipe", unet="reference", lpips_dtype=T),
             "recipe": WifStep(2, dev, objective="recipe", unet="reference")}
    sec = alternate({k: (lambda s=s: s()) for k, s in steps.items()}, warmup, rounds)
    sec["peak_bytes"] = {k: peak_above_inputs(lambda s=s: s()) for k, s in steps.items()}
    sec["terms"] = {k: {n: float(v) for n, v in s.terms.items()} for k, s in steps.items()}
    print(f"step16: recipe16 {sec['recipe16']['median_ms']:.2f} recipe {sec['recipe']['median_ms']:.2f} ms "
          f"(spread {sec['spread']:.3f})", flush=True)
    return sec


def alex16_section(dev, rounds, warmup, T):
    torch.manual_seed(0)
    fp32 = LPIPS("alex").to(dev)
    fused = LPIPS.load("alex", state=fp32.state_dict(), act_dtype=T).to(dev)
    plain = LPIPS.load("alex", state=fp32.state_dict(), fused=False, act_dtype=T).to(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    in0 = torch.rand(40, 3, 512, 1024, generator=g, device=dev) * 2 - 1
    in1 = torch.rand(40, 3, 512, 1024, generator=g, device=dev) * 2 - 1

    def run(mod):
        with torch.no_grad():
            return mod(in0, in1)

    sec = alternate({"fused16": lambda: run(fused), "framework16": lambda: run(plain), "fp32": lambda: run(fp32)},
                    warmup, rounds)
    sec["frames"], sec["chunk"] = 40, fused.chunk
    print(f"alex16 40 frames fwd: fused16 {sec['fused16']['median_ms']:.2f} framework16 {sec['framework16']['median_ms']:.2f} "
          f"fp32 {sec['fp32']['median_ms']:.2f} ms (spread {sec['spread']:.3f})", flush=True)
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="profiles/lpips.json; profiles/lpips_16bit.json with --dtype")
    ap.add_argument("--rounds", type=int, default=None, help="20; 15 with --dtype")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sections", default="level,module,step,alex")
    ap.add_argument("--dtype", choices=sorted(DTYPES), default=None,
                    help="the 16-bit sections (LPIPS.act_dtype and the waldo_lpips_level_*_dt kernels) in place of the fp32 ones")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lpips_16bit.json" if args.dtype else "lpips.json")
    if args.rounds is None:
        args.rounds = 15 if args.dtype else 20
    dev = torch.device("cuda:0")
    doc = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup)
    sections = dict(level=level_section, module=module_section, step=step_section, alex=alex_section)
    if args.dtype:
        doc["dtype"] = args.dtype
        T = DTYPES[args.dtype]
        sections = {k: (lambda d, r, w, fn=fn: fn(d, r, w, T)) for k, fn in
                    dict(level=level16_section, module=module16_section, step=step16_section, alex=alex16_section).items()}
    for name in args.sections.split(","):
        doc[name] = sections[name](dev, args.rounds, args.warmup)
        with open(args.out, "w") as fh:  # (after every section: a later one that fails loses nothing)
            json.dump(doc, fh, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
