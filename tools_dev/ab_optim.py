"""dev: the optimizer step (waldo_amd.optim) at the real parameter lists of the three recipe networks -- LVD
(tools.lvd_step.recipe_net_opt), FLP (tools.flp_step.flp_recipe_opt) and the WIF UNet (tools.wif_step.wif_opt) -- against
torch's own:

  ours                 optim.Adam(max_norm=1).step(loss): NaN test, norm, clip and update, no host read
  ours_graph           the same replayed from one captured graph
  foreach              torch.optim.Adam(foreach=True).step() alone
  foreach_ref          the reference's lines in front of it: bool(loss.isnan()) read on the host, clip_grad_norm_
  fused                torch.optim.Adam(fused=True, capturable=True).step() alone
  fused_ref            the same lines in front of it
  fused_graph          fused alone, replayed from one captured graph (clip and NaN test cannot go in: the host read)

    python tools_dev/ab_optim.py [--out profiles/optim.json] [--rounds 20] [--inner 20] [--no-flp-step]

Per list: milliseconds per step (blocks of ``inner`` steps between device events, the routes taken in alternation, one block
of each per round; median, quartiles, spread), the bytes our step needs from the sizes (28 per parameter in the update, 4
in the statistics pass) and the GB/s that makes.  Then the FLP training step at its recipe shape (4 clips of 14 frames),
eager against replayed, with and without the update in the graph.  Nothing is gated on any ratio."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from waldo_amd import optim  # noqa: E402

LR, BETAS, MAX_NORM = 1e-4, (0.0, 0.99), 1.0


def parameter_lists():
    """name -> the shapes of the network's parameters, built on the CPU at the recipe's options."""
    from waldo_amd.nets import FLP, LVD, WIF
    from waldo_amd.tools.flp_step import flp_recipe_opt
    from waldo_amd.tools.lvd_step import recipe_net_opt
    from waldo_amd.tools.wif_step import wif_opt
    nets = {"LVD": LVD(recipe_net_opt()), "FLP": FLP(flp_recipe_opt()), "WIF_UNet": WIF.with_unet(wif_opt()).unet}
    return {k: [tuple(p.shape) for p in net.parameters()] for k, net in nets.items()}


def alternate_blocks(routes, warmup, rounds, inner):
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    out = {}
    for k, v in ms.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        out[k] = dict(median_ms=round(med, 4), min_ms=round(float(np.min(v)), 4), q1_ms=round(q1, 4), q3_ms=round(q3, 4),
                      rounds=len(v), inner=inner)
    out["spread"] = round(max((s["q3_ms"] - s["q1_ms"]) / s["median_ms"] for s in out.values()), 4)
    return out


def leaves(shapes, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.nn.Parameter(0.02 * torch.randn(s, generator=g, device=dev)) for s in shapes]
    for p in ps:
        p.grad = 1e-3 * torch.randn(p.shape, generator=g, device=dev)
    return ps


def graphed(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def reference_lines(ps, opt, loss):
    """models/synthesizer.py:1057-1072 without the backward: the host read, the clip, the step."""
    if not bool(loss.isnan()):
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()


def one_list(shapes, dev, args):
    loss = torch.tensor(0.5, device=dev)
    routes = {}
    ours = optim.Adam(leaves(shapes, dev, 0), lr=LR, betas=BETAS, max_norm=MAX_NORM)
    routes["ours"] = lambda: ours.step(loss)
    ours_g = optim.Adam(leaves(shapes, dev, 0), lr=LR, betas=BETAS, max_norm=MAX_NORM)
    routes["ours_graph"] = graphed(lambda: ours_g.step(loss), dev)
    for name, kw in (("foreach", dict(foreach=True)), ("fused", dict(fused=True, capturable=True))):
        ps = leaves(shapes, dev, 0)
        opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, **kw)
        routes[name] = opt.step
        ps2 = leaves(shapes, dev, 0)
        opt2 = torch.optim.Adam(ps2, lr=LR, betas=BETAS, **kw)
        routes[name + "_ref"] = lambda ps=ps2, opt=opt2: reference_lines(ps, opt, loss)
    ps = leaves(shapes, dev, 0)
    fused_g = torch.optim.Adam(ps, lr=LR, betas=BETAS, fused=True, capturable=True)
    routes["fused_graph"] = graphed(fused_g.step, dev)
    res = alternate_blocks(routes, args.warmup, args.rounds, args.inner)
    n = sum(int(np.prod(s)) for s in shapes)
    nbytes = 32 * n
    for k, r in res.items():
        if k.startswith("ours"):
            r["GBps"] = round(nbytes / r["median_ms"] / 1e6, 1)
    return dict(tensors=len(shapes), parameters=n, launches=optim.launches_per_step(sum(1 for s in shapes if np.prod(s))),
                bytes_per_step=nbytes, largest=int(max(np.prod(s) for s in shapes)), routes=res)


def flp_step(dev, args):
    from waldo_amd.tools.flp_step import FlpStep
    kw = dict(frames=14, ctx_len=4, flp_over=dict(zero_init_dec=False))
    routes = {"eager_no_update": FlpStep(4, dev, **kw), "eager_update": FlpStep(4, dev, optimizer="adam", **kw),
              "graph_no_update": FlpStep(4, dev, graph=True, **kw),
              "graph_update": FlpStep(4, dev, graph=True, optimizer="adam", **kw)}
    res = alternate_blocks(routes, args.warmup, args.rounds, max(1, args.inner // 5))
    res["parameters"] = sum(p.numel() for p in routes["graph_update"].leaves)
    res["skipped"] = float(routes["graph_update"].optimizer.skipped)
    res["steps"] = float(routes["graph_update"].optimizer.step_count)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-flp-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_optim.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, limits=optim.limits(),
               hyper=dict(lr=LR, betas=BETAS, max_norm=MAX_NORM), method=__doc__.split("\n\n")[-1], lists={})
    for name, shapes in parameter_lists().items():
        doc["lists"][name] = one_list(shapes, dev, args)
        print(name, json.dumps(doc["lists"][name]["routes"]), flush=True)
        torch.cuda.empty_cache()
    if not args.no_flp_step:
        doc["flp_step"] = flp_step(dev, args)
        print("flp_step", json.dumps(doc["flp_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
