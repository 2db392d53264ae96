"""A/B of the LPIPS level kernel (``WF.lpips_level``, include/waldo_hip.h "LPIPS level distance") against the chain of
framework ops it replaces (``WF.lpips_level_framework``), of the ``LPIPS`` module with either, and of the WIF training
step with and without the recipe's ``lpips_vid`` term, on one MI355X.  Writes profiles/lpips.json.

    python tools_dev/ab_lpips.py [--out profiles/lpips.json] [--rounds 20] [--warmup 3] [--sections level,module,step,alex]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sections", default="level,module,step,alex")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup)
    sections = dict(level=level_section, module=module_section, step=step_section, alex=alex_section)
    for name in args.sections.split(","):
        doc[name] = sections[name](dev, args.rounds, args.warmup)
        with open(args.out, "w") as fh:  # (after every section: a later one that fails loses nothing)
            json.dump(doc, fh, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
