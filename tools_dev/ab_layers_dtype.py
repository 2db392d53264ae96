"""dev: the fused warp/composite with an fp32, bf16 and fp16 layer stack, interleaved, with bench.py's protocol (settle,
warm-up, five timed blocks bracketed by synchronize, median).  C3: the training step (bench.synth, seed 0, sigma 0.05,
rgb.square().mean().backward()); C5: the forward.  Per variant: ms per step, the entry points' event time per step,
and the step's peak device memory (its inputs plus what it allocates).  One JSON line per variant, also written to
OUT/r10_layers_dtype_<config>_<dtype>.json.

    python tools_dev/ab_layers_dtype.py [--steps 20] [--warmup 5] [--only bf16] [--config C3 C5] [--out profiles]
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

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def variant(config, dtype, dev):
    clips, fpc, nl, h, w, mode = bench.CONFIGS[config]
    tps = waldo_amd.TPSWarp(h, w, get_grid(4, 4).view(-1, 2)).to(dev)
    layers, pts, occ = bench.synth(clips * fpc, nl, h, w, dev, seed=0, sigma=0.05)
    layers = layers.to(dtype)
    train = mode == "train"
    if train:
        layers.requires_grad_()
        pts.requires_grad_()

    def step():
        if train:
            layers.grad = None
            pts.grad = None
            rgb = WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)
            rgb.square().mean().backward()
        else:
            with torch.no_grad():
                WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)

    return step, layers


def fence():
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["C3", "C5"], choices=["C3", "C5"])
    ap.add_argument("--only", choices=sorted(DTYPES), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", default=None, help="another build of the library")
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    dev = torch.device("cuda:0")
    names = [args.only] if args.only else list(DTYPES)
    os.makedirs(args.out, exist_ok=True)
    for config in args.config:
        runs = {n: variant(config, DTYPES[n], dev) for n in names}
        settle = {}
        for n, (step, _) in runs.items():
            for _ in range(3):
                step()
            settle[n] = bench.settle_gpu(step, fence)
            for _ in range(args.warmup):
                step()
        bench.settle_interpreter()
        blocks = {n: [] for n in names}
        for _ in range(bench.TIMED_BLOCKS):  # interleaved: one block of each variant in turn
            for n, (step, _) in runs.items():
                blocks[n] += bench.timed_blocks(step, fence, args.steps, nblocks=1)
        for n, (step, layers) in runs.items():
            with _lib.KernelTimer() as kt:
                step()
                fence()
            entry = {k: round(v[1] * v[0], 4) for k, v in kt.summary().items()}
            if layers.grad is not None:
                layers.grad = None
            fence()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step()
            fence()
            peak = torch.cuda.max_memory_allocated() - base + layers.numel() * layers.element_size()
            line = {"variant": f"{config}_{n}", "lib": os.path.basename(_lib.LIB_PATH), "config": config,
                    "layers_dtype": n, "ms_per_step": round(bench.median_block(blocks[n]) / args.steps * 1e3, 4),
                    "ms_per_step_blocks": [round(b / args.steps * 1e3, 4) for b in blocks[n]],
                    "settle_ms": settle[n], "entry_ms_per_step": entry, "step_peak_bytes": int(peak),
                    "timing": f"median of {bench.TIMED_BLOCKS} blocks of {args.steps} steps, the variants interleaved "
                              f"block by block, after settling and {args.warmup} warm-up steps"}
            print(json.dumps(line), flush=True)
            with open(os.path.join(args.out, f"r10_layers_dtype_{config}_{n}.json"), "w") as fh:
                fh.write(json.dumps(line) + "\n")
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
