"""Score predicted clips against the real ones: PSNR, SSIM, MS-SSIM and LPIPS per frame on the GPU.

    python -m waldo_amd.tools.evaluate REAL FAKE VID_LENGTH VID_CONTEXT [--metrics psnr ssim msssim lpips]
                                       [--batch-size 16] [--drop-last] [--json PATH]
                                       [--lpips-net alex|vgg] [--lpips-state FILE | --lpips-backbone FILE --lpips-lin FILE]
                                       [--lpips-dtype bf16|fp16]

Step 2 of the reference's evaluation (tools/eval/metrics.py, README "Metrics").  REAL and FAKE are directories of
clips as ``tools.io.dump_video`` writes them: one sub-directory of PNG frames, or one APNG / WebP / GIF file, per clip.
Clips are paired by sorted name and the counts must match (metrics.py:90-92); each clip's first VID_LENGTH frames are
scored through the uint8 path of ``waldo_amd.metrics.frame_metrics``, batch by batch.  Printed: the reference's running
``[name:t] : mean`` lines per batch, then ``[name:t] : (mean, std)`` per t and ``[cum name:t] : (mean, std)`` over the
frames VID_CONTEXT..t (metrics.py:95-113).

LPIPS (the reference's default metric next to MS-SSIM, metrics.py:127: AlexNet with the lin layers) is scored when its
weights are given: ``--lpips-state``, a saved ``lpips.LPIPS`` state dict, or ``--lpips-backbone`` (torchvision's
``alexnet`` / ``vgg16`` state dict) with ``--lpips-lin`` (the package's ``weights/v0.1/alex.pth`` / ``vgg.pth``).  No
pretrained weights ship with this library, and its LPIPS has not been compared with the package's outputs.

Differences from the reference: no mp4 (no decoder), no ``--compress`` / ``--resize`` (cv2's INTER_LINEAR).  The reference scores ``total_size // batch_size`` batches and so
drops a last partial batch (metrics.py:97); this tool scores every clip unless ``--drop-last`` is given, and says so when
the two counts differ.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from .. import metrics as M
from . import io as wio

CLIP_EXT = (".png", ".webp", ".gif")


def clip_paths(folder):
    """The clips under ``folder``, sorted by name: PNG-frame directories and animation files."""
    if not os.path.isdir(folder):
        raise ValueError(f"evaluate: {folder} is not a directory")
    names = sorted(os.listdir(folder))
    return [os.path.join(folder, n) for n in names
            if os.path.isdir(os.path.join(folder, n)) or n.lower().endswith(CLIP_EXT)]


def load_batch(paths, vid_length):
    clips = []
    for p in paths:
        v = wio.load_video_u8(p)
        if v.shape[0] < vid_length:
            raise ValueError(f"evaluate: {p} has {v.shape[0]} frames, VID_LENGTH is {vid_length}")
        clips.append(v[:vid_length])
    if any(c.shape != clips[0].shape for c in clips):
        raise ValueError("evaluate: the clips of a batch differ in frame size")
    return torch.stack(clips)


LPIPS_DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}  # --lpips-dtype


def lpips_module(net="alex", state=None, backbone=None, lin=None, device="cuda:0", act_dtype=None):
    """The ``LPIPS`` module of the ``--lpips-*`` arguments on ``device``, or None when no file is given.  ``act_dtype``:
    ``LPIPS.act_dtype`` (the backbone under autocast, the 16-bit level kernels)."""
    if state is None and backbone is None and lin is None:
        return None
    from ..nets import LPIPS
    return LPIPS.load(net, state=state, backbone=backbone, lin=lin, act_dtype=act_dtype).to(torch.device(device))


def evaluate(real_dir, fake_dir, vid_length, vid_context, metrics=M.METRICS, batch_size=16, drop_last=False,
             device="cuda:0", out=sys.stdout, lpips=None):
    """Scores (name -> (clips, vid_length) float64 numpy) and their ``metrics.summarize``; prints as the reference.
    ``lpips``: an ``LPIPS`` module on ``device`` (``lpips_module``); with it ``"lpips"`` may be among ``metrics``."""
    metrics = M.check_metrics(metrics, lpips)
    real, fake = clip_paths(real_dir), clip_paths(fake_dir)
    if len(real) != len(fake):
        raise ValueError(f"evaluate: {len(real)} real clips and {len(fake)} predicted clips")
    total = len(real)
    n = (total // batch_size) * batch_size if drop_last else total
    if n != (total // batch_size) * batch_size:
        print(f"note: scoring all {total} clips; the reference scores {(total // batch_size) * batch_size} "
              f"(whole batches of {batch_size} only: --drop-last)", file=out)
    dev = torch.device(device)
    scores = {m: [] for m in metrics}
    for start in range(0, n, batch_size):
        end = min(start + batch_size, n)
        r = load_batch(real[start:end], vid_length).to(dev)
        f = load_batch(fake[start:end], vid_length).to(dev)
        res = M.frame_metrics(f, r, metrics=metrics, lpips=lpips)
        for m in metrics:
            scores[m].append(res[m].double().cpu().numpy())
        for t in range(vid_length):
            for m in metrics:
                seen = np.concatenate(scores[m])[:, t]
                print(f"[{m}:{t}] : {float(np.mean(seen))}", file=out)
    scores = {m: np.concatenate(v) if v else np.zeros((0, vid_length)) for m, v in scores.items()}
    summary = M.summarize(scores, vid_context)
    for line in M.format_lines(summary):
        print(line, file=out)
    return scores, summary


def add_lpips_arguments(ap):
    ap.add_argument("--lpips-net", choices=("alex", "vgg"), default="alex",
                    help="the LPIPS backbone (alex: the reference's evaluation)")
    ap.add_argument("--lpips-state", default=None, help="a saved lpips.LPIPS state dict")
    ap.add_argument("--lpips-backbone", default=None, help="torchvision's alexnet / vgg16 state dict (with --lpips-lin)")
    ap.add_argument("--lpips-lin", default=None, help="the lpips package's lin-layer file (with --lpips-backbone)")
    ap.add_argument("--lpips-dtype", choices=sorted(LPIPS_DTYPES), default="fp32",
                    help="bf16 / fp16: the LPIPS backbone under autocast and the 16-bit level kernels (LPIPS.act_dtype)")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("real", help="directory of the real clips")
    ap.add_argument("fake", help="directory of the predicted clips")
    ap.add_argument("vid_length", type=int)
    ap.add_argument("vid_context", type=int)
    ap.add_argument("--metrics", nargs="+", default=list(M.METRICS),
                    help="psnr, ssim, msssim; lpips with --lpips-state or --lpips-backbone and --lpips-lin")
    add_lpips_arguments(ap)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--drop-last", action="store_true",
                    help="score whole batches only, as the reference does (metrics.py:97)")
    ap.add_argument("--json", default=None, help="write metrics.summarize's result here")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be >= 1")
    lpips = lpips_module(args.lpips_net, args.lpips_state, args.lpips_backbone, args.lpips_lin, args.device,
                         act_dtype=LPIPS_DTYPES[args.lpips_dtype])
    _, summary = evaluate(args.real, args.fake, args.vid_length, args.vid_context, metrics=tuple(args.metrics),
                          batch_size=args.batch_size, drop_last=args.drop_last, device=args.device, lpips=lpips)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
