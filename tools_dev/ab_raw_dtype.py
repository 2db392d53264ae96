"""dev: the 16-bit WIF input on the C5 pipeline (raw_dtype fp32 / bf16 / fp16, eager, same seeds, interleaved rounds)
and wif_fuse alone at the C5 WIF shape for every (vid, net) dtype pair.  One JSON line per variant.

    python tools_dev/ab_raw_dtype.py [--steps 5] [--warmup 2] [--only bf16] [--no-wif]

(--only: one pipeline variant and nothing else -- for rocprofv3 runs, `rocprofv3 ... -- python tools_dev/ab_raw_dtype.py
--only bf16 --no-wif --steps 2 --warmup 1`.)"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from waldo_amd import _lib  # noqa: E402
from waldo_amd import functional as WF  # noqa: E402
from waldo_amd.tools import demo  # noqa: E402
from waldo_amd.tools.pipeline import Pipeline  # noqa: E402

DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def time_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=sorted(DTYPES), default=None)
    ap.add_argument("--no-wif", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (tools_dev/build_variant.py)")
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    dev = torch.device("cuda:0")
    pipe = Pipeline("C5", 4, dev, seed=0)
    opt, ctx_len = pipe.opt, pipe.ctx_len

    def step(dt):
        return demo.predict(opt, pipe.warper, pipe.wif, pipe.vid, pipe.lyt, pipe.net, ctx_len, raw_dtype=dt)

    names = [args.only] if args.only else list(DTYPES)
    res = {n: {"ms": [], "entry_ms": {}} for n in names}
    for _ in range(1 if args.only else args.rounds):
        for n in names:
            with torch.no_grad():
                res[n]["ms"].append(time_ms(lambda: step(DTYPES[n]), args.steps, args.warmup))
    for n in names:  # per entry point (event pairs around every C-ABI call), one more step each
        with torch.no_grad(), _lib.KernelTimer() as kt:
            step(DTYPES[n])
            torch.cuda.synchronize()
        res[n]["entry_ms"] = {k: round(v[1] * v[0], 3) for k, v in kt.summary().items()
                              if "frame_warp_fuse" in k or "flow_ctx_warp" in k or "wif_fuse" in k}
        print(json.dumps({"variant": "pipeline_C5", "lib": os.path.basename(_lib.LIB_PATH), "raw_dtype": n, "ms_per_step": min(res[n]["ms"]),
                          "ms_rounds": [round(x, 3) for x in res[n]["ms"]], "entry_ms_per_step": res[n]["entry_ms"]}))
    del pipe
    torch.cuda.empty_cache()
    if args.only or args.no_wif:
        return
    # wif_fuse alone at the C5 WIF shape: the 10 predicted frames of a clip, Tc = 4, C + L = 15, 512 x 1024
    g = torch.Generator(device=dev).manual_seed(0)
    vid32 = torch.rand(1, 10, 4, 15, 512, 1024, generator=g, device=dev) * 2 - 1
    net32 = torch.randn(1, 10, 4, 4, 512, 1024, generator=g, device=dev)
    for vn, vdt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
        for nn_, ndt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
            vid, net = vid32.to(vdt), net32.to(ndt)
            with torch.no_grad():
                ms = time_ms(lambda: WF.wif_fuse(vid, net), 10, 3)
            v2, n2 = vid.clone().requires_grad_(), net.clone().requires_grad_()
            out = WF.wif_fuse(v2, n2)
            go = torch.ones_like(out)
            ms_b = time_ms(lambda: torch.autograd.grad(out, (v2, n2), go, retain_graph=True), 5, 2)
            print(json.dumps({"variant": "wif_fuse_C5", "vid": vn, "net": nn_, "fwd_ms": round(ms, 3),
                              "bwd_ms": round(ms_b, 3)}))
            del vid, net, v2, n2, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
