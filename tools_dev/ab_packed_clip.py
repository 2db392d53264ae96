"""dev: the packed clip on the C5 pipeline -- demo.predict on the fp32 clip (vid + lyt, 23 fp32 planes) against the same
clip packed (functional.PackedClip: RGB bytes + class id, one word per pixel), each with raw_dtype fp32 and bf16; eager,
same seeds, interleaved rounds.  The two inputs hold the same data (the fp32 clip is the packed one's unpack()), and the
first step of every raw dtype checks that both give the same outputs bit for bit.  One JSON line per variant.

    python tools_dev/ab_packed_clip.py [--steps 5] [--warmup 2] [--rounds 2] [--only packed-bf16] [--lib OTHER.so]

(--only: one variant and nothing else -- for rocprofv3 runs, `rocprofv3 --kernel-trace --stats ... -- python
tools_dev/ab_packed_clip.py --only packed-bf16 --steps 2 --warmup 1`, and `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` in runs
of their own.)"""
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

VARIANTS = {"fp32clip-fp32": (False, None), "packed-fp32": (True, None),
            "fp32clip-bf16": (False, torch.bfloat16), "packed-bf16": (True, torch.bfloat16)}
ENTRIES = ("frame_warp_fuse", "flow_ctx_alpha", "downscale_frames", "unpack_clip")


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
    ap.add_argument("--only", choices=sorted(VARIANTS), default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (tools_dev/build_variant.py)")
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    dev = torch.device("cuda:0")
    pipe = Pipeline("C5", 4, dev, seed=0)
    opt, ctx_len = pipe.opt, pipe.ctx_len
    # the pipeline's piecewise-constant class map, random RGB bytes; the fp32 clip is the packed clip's unpacked form
    g = torch.Generator(device=dev).manual_seed(0)
    b, t, _, hd, wd = pipe.vid.shape
    rgb = torch.randint(0, 256, (b, t, 3, hd, wd), generator=g, device=dev, dtype=torch.uint8)
    packed = WF.pack_clip(rgb, pipe.lyt.argmax(dim=2), opt.num_lyt)
    del pipe.vid, pipe.lyt
    names = [args.only] if args.only else list(VARIANTS)
    if any(not VARIANTS[n][0] for n in names):
        full = packed.unpack()
        vid, lyt = full[:, :, :3], full[:, :, 3:]

    def step(name):
        is_packed, dt = VARIANTS[name]
        if is_packed:
            return demo.predict(opt, pipe.warper, pipe.wif, packed, None, pipe.net, ctx_len, raw_dtype=dt)
        return demo.predict(opt, pipe.warper, pipe.wif, vid, lyt, pipe.net, ctx_len, raw_dtype=dt)

    same = {}
    if not args.only:
        with torch.no_grad():
            for dt_name in ("fp32", "bf16"):
                r0 = step("fp32clip-" + dt_name)
                r0 = {k: v.clone() for k, v in r0.items()}
                r1 = step("packed-" + dt_name)
                same[dt_name] = set(r0) == set(r1) and all(torch.equal(r0[k], r1[k]) for k in r0)
                del r0, r1
    res = {n: [] for n in names}
    for _ in range(1 if args.only else args.rounds):
        for n in names:
            with torch.no_grad():
                res[n].append(time_ms(lambda: step(n), args.steps, args.warmup))
    for n in names:  # per entry point (event pairs around every C-ABI call), one more step each
        with torch.no_grad(), _lib.KernelTimer() as kt:
            step(n)
            torch.cuda.synchronize()
        entry = {k: round(v[1] * v[0], 3) for k, v in kt.summary().items() if any(e in k for e in ENTRIES)}
        line = {"variant": "pipeline_C5", "lib": os.path.basename(_lib.LIB_PATH), "clip": "packed" if VARIANTS[n][0] else "fp32",
                "raw_dtype": n.split("-")[1], "ms_per_step": round(min(res[n]), 3),
                "ms_rounds": [round(x, 3) for x in res[n]], "entry_ms_per_step": entry,
                "clip_bytes": packed.data.numel() if VARIANTS[n][0] else 4 * b * t * (3 + opt.num_lyt) * hd * wd}
        if same:
            line["same_outputs_as_fp32_clip"] = same[n.split("-")[1]]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
