"""dev: what byte output (``out_bytes``, include/waldo_hip.h "Byte output") costs and saves, at the Cityscapes recipe's
``predict`` shape (C5: 4 clips x 14 frames, 512 x 1024, Tc = 4, 12 layers, stand-in networks) and at the WIF recipe's
fusion shape (40-channel ``raw_output``, 5-channel network output, Tc = 4, 10 frames of 512 x 1024):

  (a) ``wif_fuse`` (fp32 out, as before) against ``wif_fuse_bytes`` -- the keep-or-drop rule of the fused epilogue: it
      must be no slower than ``wif_fuse`` beyond the spread of the 7 ``wif_fuse`` samples of the same session;
  (b) the routes to the dumped bytes: ``wif_fuse`` + the framework's quantise chain (clamp, sub, div, mul, cast: the only
      route before), ``wif_fuse`` + ``frames_to_bytes``, ``wif_fuse_bytes``;
  (c) ``predict`` and the copy of its six image outputs to pinned host memory, fp32 against ``out_bytes="trunc"``;
  (d) the bytes (c) moves in each form.

The forms of a group are interleaved in ONE process, timed with events on the launch stream, median of 7 after 3
warm-ups (best and worst reported with it).  One GPU process: run it under a time limit,

    timeout -k 10 600 python tools_dev/ab_out_bytes.py [--out profiles/out_bytes.json] [--clips 4] [--lib PATH]"""
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

IMAGE_KEYS = ("rec_vid", "inp_rec_vid", "pred_vid", "inp_pred_vid", "rec_disocc", "pred_disocc")
REPS, WARMUP = 7, 3


def torch_bytes(x, lo=-1.0, hi=1.0):
    """The reference's expression (tools/utils.py:246-264) as framework ops: five launches over the clip."""
    return ((x.clamp(lo, hi) - lo) / (hi - lo) * 255).to(torch.uint8)


def interleaved(forms):
    """{name: fn} -> {name: sorted ms of REPS event-timed calls}, the forms taking turns."""
    for _ in range(WARMUP):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in forms}
    for _ in range(REPS):
        for n, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    return {n: sorted(v) for n, v in ms.items()}


def stats(ts):
    return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}


def fusion_groups(vid, net):
    a = interleaved({"wif_fuse": lambda: WF.wif_fuse(vid, net),
                     "wif_fuse_bytes": lambda: WF.wif_fuse_bytes(vid, net)})
    b = interleaved({"wif_fuse+torch_chain": lambda: torch_bytes(WF.wif_fuse(vid, net)),
                     "wif_fuse+frames_to_bytes": lambda: WF.frames_to_bytes(WF.wif_fuse(vid, net)),
                     "wif_fuse_bytes": lambda: WF.wif_fuse_bytes(vid, net)})
    same = torch.equal(WF.wif_fuse_bytes(vid, net), WF.frames_to_bytes(WF.wif_fuse(vid, net)))
    px = vid.shape[0] * vid.shape[1] * vid.shape[-2] * vid.shape[-1]
    spread = a["wif_fuse"][-1] - a["wif_fuse"][0]
    return {"shape": {"vid": list(vid.shape), "net": list(net.shape), "dtype": str(vid.dtype).split(".")[-1]},
            "pixels": px, "bytes_equal_two_launches": bool(same),
            "a": {n: stats(t) for n, t in a.items()},
            "a_rule": {"wif_fuse_spread_ms": round(spread, 4),
                       "fused_minus_parent_ms": round(a["wif_fuse_bytes"][REPS // 2] - a["wif_fuse"][REPS // 2], 4),
                       "keep_fused": bool(a["wif_fuse_bytes"][REPS // 2] <= a["wif_fuse"][REPS // 2] + spread)},
            "b": {n: stats(t) for n, t in b.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join("profiles", "out_bytes.json"))
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--lib", default=None, help="another build of the library, timed under this script")
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(args.lib)
    dev = torch.device("cuda:0")
    doc = {"what": f"byte output at C5 predict ({args.clips} clips x 14 frames, 512x1024, Tc=4, 12 layers, stand-in "
                   "networks) and at the WIF recipe's fusion (40-channel raw_output, Tc=4, 10 frames of 512x1024)",
           "how": f"forms of a group interleaved in one process, event-timed, median of {REPS} after {WARMUP} warm-ups",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # ---- C5 predict: the fusion's own inputs are taken from a predict() call
        pipe = Pipeline("C5", args.clips, dev, seed=5)
        seen = {}
        fuse = pipe.wif.fuse

        def grab(vid_t, net_out, out_bytes=None):
            seen["vid"], seen["net"] = vid_t, net_out
            return fuse(vid_t, net_out, out_bytes=out_bytes)

        pipe.wif.fuse = grab
        pipe()
        pipe.wif.fuse = fuse
        doc["fusion_C5"] = fusion_groups(seen["vid"], seen["net"])
        seen.clear()

        # ---- (c), (d): predict + the six image outputs to pinned host memory
        def run(out_bytes):
            return demo.predict(pipe.opt, pipe.warper, pipe.wif, pipe.vid, pipe.lyt, pipe.net, pipe.ctx_len,
                                out_bytes=out_bytes)

        host = {}
        for form, ob in (("fp32", None), ("bytes_trunc", "trunc")):
            res = run(ob)
            host[form] = {k: torch.empty(res[k].shape, dtype=res[k].dtype).pin_memory() for k in IMAGE_KEYS}
            del res

        def predict_and_copy(form, ob):
            res = run(ob)
            for k in IMAGE_KEYS:
                host[form][k].copy_(res[k], non_blocking=True)

        c = interleaved({"fp32": lambda: predict_and_copy("fp32", None),
                         "bytes_trunc": lambda: predict_and_copy("bytes_trunc", "trunc")})
        only = interleaved({"fp32": lambda: run(None), "bytes_trunc": lambda: run("trunc")})
        same = all(torch.equal(host["bytes_trunc"][k], WF.frames_to_bytes(run(None)[k]).cpu()) for k in IMAGE_KEYS)
        doc["predict_C5"] = {
            "c_predict_and_copy_to_pinned_host": {n: stats(t) for n, t in c.items()},
            "predict_alone": {n: stats(t) for n, t in only.items()},
            "d_bytes_of_the_six_image_outputs": {form: int(sum(v.numel() * v.element_size() for v in host[form].values()))
                                                 for form in host},
            "bytes_equal_quantised_fp32": bool(same)}
        del pipe, host
        torch.cuda.empty_cache()

        # ---- the WIF recipe's fusion shape
        g = torch.Generator(device=dev).manual_seed(3)
        vid = torch.randn(1, 10, 4, 40, 512, 1024, generator=g, device=dev)
        net = torch.randn(1, 10, 4, 5, 512, 1024, generator=g, device=dev) * 0.5
        doc["fusion_WIF_recipe"] = fusion_groups(vid, net)
        doc["fusion_WIF_recipe_bf16"] = fusion_groups(vid.bfloat16(), net.bfloat16())
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
