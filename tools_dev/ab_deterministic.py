"""dev: what deterministic mode costs.  The default and the deterministic backward of the same step, alternated block by
block in one process with bench.py's protocol (settle, warm-up, five timed blocks bracketed by synchronize, median):

    LVD        the warp-path part of an LVD training step (waldo_amd/tools/lvd_step.py), eager
    LVD_graph  the same step captured into a HIP graph and replayed
    HD         forward + full-resolution backward of decode_output at the Cityscapes recipe's size (128 x 256 upsampled
               x4 to 512 x 1024, 16 objects, 20 layout classes, 5 frames, ctx_mode "prev", include_self)
    C3         the fused warp/composite's training step (bench.synth, seed 0) with a gradient on occ

Per variant: ms per step, the entry points' event time per step, the deterministic workspaces' bytes per step and the
step's peak device memory.  One JSON line per variant, also written to OUT/r11_deterministic_<config>_<mode>.json.

    python tools_dev/ab_deterministic.py [--steps 20] [--warmup 5] [--config LVD LVD_graph HD C3] [--out profiles]
                                         [--lib OTHER/libwaldo_hip.so]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import waldo_amd  # noqa: E402
from waldo_amd import _lib  # noqa: E402
from waldo_amd import functional as WF  # noqa: E402
from waldo_amd.tools.utils import get_grid  # noqa: E402

MODES = {"default": False, "det": True}


def lvd(dev, det, graph):
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(2, dev, seed=0)

    def run():
        with WF.deterministic(det):
            step()

    if not graph:
        return run
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g.replay


def hd(dev, det):
    from waldo_amd.nets import Warper, decode_output, estimate_alpha_grid_occ
    from waldo_amd.tools.lvd_step import lvd_opt
    opt = lvd_opt(load_dim=512)
    wp = Warper(opt).to(dev)
    b, t, no, nl = 1, 5, opt.num_obj, 20
    lo, lb = opt.obj_shape[0] * opt.obj_shape[1], opt.latent_shape[0] * opt.latent_shape[1]
    h, w, ho = opt.dim, opt.dim * opt.aspect_ratio, opt.obj_shape[0] * opt.patch_size
    g = torch.Generator(device=dev).manual_seed(0)
    obj_alpha = (torch.rand(b, no, 1, ho, ho, generator=g, device=dev) * 2 - 1).requires_grad_()
    obj_pose = (get_grid(*opt.obj_shape).view(1, 1, 1, lo, 2).to(dev) * 0.5
                + 0.15 * torch.randn(b, t, no, lo, 2, generator=g, device=dev)).requires_grad_()
    bg_pose = (get_grid(*opt.latent_shape).view(1, 1, 1, lb, 2).to(dev)
               + 0.05 * torch.randn(b, t, 1, lb, 2, generator=g, device=dev)).requires_grad_()
    score = torch.randn(b, t, no, generator=g, device=dev, requires_grad=True)
    cls = torch.randn(b, no, nl, generator=g, device=dev, requires_grad=True)
    inp = torch.randn(b, t, 3 + nl, h * 4, w * 4, generator=g, device=dev)
    bg_alpha = torch.ones(1, 1, h, w, device=dev)
    ctx_ts = torch.roll(torch.arange(t, device=dev), 1).view(1, 1, t).expand(b, -1, -1).contiguous()
    pred_ts = WF.arange_index(t, dev)
    leaves = [obj_alpha, obj_pose, bg_pose, score, cls]

    def run():
        with WF.deterministic(det):
            for x in leaves:
                x.grad = None
            occ, oa, ba, grid = estimate_alpha_grid_occ(wp, obj_alpha, bg_alpha, obj_pose, bg_pose, score)
            out = decode_output(wp, inp, grid, occ, oa, ba, cls.softmax(-1), ctx_ts, pred_ts, restrict_to_ctx=False)
            (out[0].square().mean() + out[1].square().mean() + out[3].mean()).backward()

    return run


def c3(dev, det):
    clips, fpc, nl, h, w, _ = bench.CONFIGS["C3"]
    tps = waldo_amd.TPSWarp(h, w, get_grid(4, 4).view(-1, 2)).to(dev)
    layers, pts, occ = bench.synth(clips * fpc, nl, h, w, dev, seed=0, sigma=0.05)
    leaves = [layers.requires_grad_(), pts.requires_grad_(), occ.requires_grad_()]

    def run():
        with WF.deterministic(det):
            for x in leaves:
                x.grad = None
            WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t).square().mean().backward()

    return run


BUILD = {"LVD": lambda dev, det: lvd(dev, det, False), "LVD_graph": lambda dev, det: lvd(dev, det, True), "HD": hd,
         "C3": c3}


def fence():
    torch.cuda.synchronize()


def workspace_bytes(step):
    """Bytes the *_det_workspace_bytes queries of one step add up to."""
    total, query = [0], _lib.query

    def rec(name, *args):
        n = query(name, *args)
        total[0] += max(int(n), 0) if name.endswith("_det_workspace_bytes") else 0
        return n

    _lib.query = rec
    try:
        step()
        fence()
    finally:
        _lib.query = query
    return total[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=list(BUILD), choices=list(BUILD))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", help="another build of libwaldo_hip.so (the whole run uses it)")
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    for config in args.config:
        runs = {n: BUILD[config](dev, det) for n, det in MODES.items()}
        settle = {}
        for n, step in runs.items():
            for _ in range(3):
                step()
            settle[n] = bench.settle_gpu(step, fence)
            for _ in range(args.warmup):
                step()
        bench.settle_interpreter()
        blocks = {n: [] for n in runs}
        for _ in range(bench.TIMED_BLOCKS):  # interleaved: one block of each mode in turn
            for n, step in runs.items():
                blocks[n] += bench.timed_blocks(step, fence, args.steps, nblocks=1)
        lines = {}
        for n, step in runs.items():
            entry, ws = {}, 0
            if config != "LVD_graph":  # (a replay makes no library call on the host)
                with _lib.KernelTimer() as kt:
                    step()
                    fence()
                entry = {k: round(v[1] * v[0], 4) for k, v in kt.summary().items()}
                ws = workspace_bytes(step)
            fence()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step()
            fence()
            lines[n] = {"variant": f"{config}_{n}", "config": config, "mode": n,
                        "ms_per_step": round(bench.median_block(blocks[n]) / args.steps * 1e3, 4),
                        "ms_per_step_blocks": [round(b / args.steps * 1e3, 4) for b in blocks[n]],
                        "settle_ms": settle[n], "entry_ms_per_step": entry, "det_workspace_bytes_per_step": ws,
                        "step_peak_bytes_over_resident": int(torch.cuda.max_memory_allocated() - base),
                        "timing": f"median of {bench.TIMED_BLOCKS} blocks of {args.steps} steps, the two modes "
                                  f"interleaved block by block, after settling and {args.warmup} warm-up steps"}
        lines["det"]["ratio_to_default"] = round(lines["det"]["ms_per_step"] / lines["default"]["ms_per_step"], 3)
        for n, line in lines.items():
            print(json.dumps(line), flush=True)
            with open(os.path.join(args.out, f"r11_deterministic_{config}_{n}.json"), "w") as fh:
                fh.write(json.dumps(line) + "\n")
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
