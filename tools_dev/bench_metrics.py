"""Frame metrics (waldo_amd.metrics.frame_metrics) at the C5 prediction's frames, 4 clips x 10 frames x 3 x 512 x 1024,
PSNR + SSIM + MS-SSIM, against the same formulas in eager PyTorch (grouped F.conv2d with the 11 x 11 window).

    python tools_dev/bench_metrics.py [--blocks 15 --per-block 5 --warmup 3] [--only fp32-packed|u8-u8|eager]

Cases: fp32 against a PackedClip (what demo --eval does), uint8 against uint8 (what tools.evaluate does), and the eager
baseline on the uint8 frames.  Event-timed: ``--blocks`` blocks of ``--per-block`` calls each, interleaved across the
cases; the median and spread of the per-call time of the blocks.  One JSON line per case (profiles/r09_metrics_*).
Checks first that the eager baseline and the kernels agree (|diff| <= 1e-4 on SSIM / MS-SSIM, 1e-3 dB on PSNR)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waldo_amd import functional as WF  # noqa: E402
from waldo_amd.metrics import frame_metrics  # noqa: E402

B, T, H, W = 4, 10, 512, 1024
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def eager_metrics(x, y):
    """PSNR, SSIM and MS-SSIM of (N, 3, H, W) fp32 [0, 1] frames in eager PyTorch: TF's definitions."""
    i = torch.arange(11, dtype=torch.float64, device=x.device)
    g = torch.exp(-0.5 * (i - 5) ** 2 / 1.5 ** 2)
    g = (g / g.sum()).float()
    win = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def ssim_cs(a, b):
        mx, my = F.conv2d(a, win, groups=3), F.conv2d(b, win, groups=3)
        num0 = mx * my * 2.0
        den0 = mx * mx + my * my
        lum = (num0 + c1) / (den0 + c1)
        num1 = F.conv2d(a * b, win, groups=3) * 2.0
        den1 = F.conv2d(a * a + b * b, win, groups=3)
        cs = (num1 - num0 + c2) / (den1 - den0 + c2)
        return (lum * cs).mean(dim=(2, 3)), cs.mean(dim=(2, 3))

    psnr = -10.0 * torch.log10(((x - y) ** 2).mean(dim=(1, 2, 3)))
    s0, cs0 = ssim_cs(x, y)
    prod = torch.relu(cs0) ** WEIGHTS[0]
    a, b = x, y
    for k in range(1, 5):
        ph, pw = a.shape[2] % 2, a.shape[3] % 2
        if ph or pw:
            a = F.pad(a, (0, pw, 0, ph), mode="replicate")  # one row / column: SYMMETRIC = replicate
            b = F.pad(b, (0, pw, 0, ph), mode="replicate")
        a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
        s, cs = ssim_cs(a, b)
        prod = prod * torch.relu(s if k == 4 else cs) ** WEIGHTS[k]
    return {"psnr": psnr, "ssim": s0.mean(dim=1), "msssim": prod.mean(dim=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--per-block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    real_u8 = torch.randint(0, 256, (B, T, 3, H, W), dtype=torch.uint8, device=dev, generator=g)
    real_u8 = torch.nn.functional.avg_pool2d(real_u8.view(-1, 1, H, W).float(), 5, 1, 2).to(torch.uint8).view(B, T, 3, H, W)
    noise = torch.randn(B, T, 3, H, W, device=dev, generator=g) * 0.05
    pred = (real_u8.float() / 127.5 - 1.0 + noise).clamp_(-1.0, 1.0)  # a prediction in [-1, 1]
    pred_u8 = ((pred + 1.0) / 2.0 * 255.0).to(torch.uint8)
    packed = WF.pack_clip(real_u8, torch.zeros(B, T, H, W, dtype=torch.uint8, device=dev), 20)
    unit = lambda u: u.view(B * T, 3, H, W).float() / 255.0  # noqa: E731
    xu, yu = unit(pred_u8), unit(real_u8)
    cases = {
        "fp32-packed": lambda: frame_metrics(pred, packed),
        "u8-u8": lambda: frame_metrics(pred_u8, real_u8),
        "eager": lambda: eager_metrics(xu, yu),
    }
    # agreement (uint8 frames: the same inputs on both sides)
    k, e = cases["u8-u8"](), cases["eager"]()
    diff = {m: (k[m].view(-1).double() - e[m].double()).abs().max().item() for m in k}
    assert diff["psnr"] <= 1e-3 and diff["ssim"] <= 1e-4 and diff["msssim"] <= 1e-4, diff
    if args.only:
        cases = {args.only: cases[args.only]}
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in cases}
    for _ in range(args.blocks):
        for n, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.per_block):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[n].append(a.elapsed_time(b) / args.per_block)
    # bytes the kernels must read: the two operands once at scale 0 (fp32: 4 B, uint8: 1 B, packed: 4 B per pixel)
    px = B * T * H * W
    read = {"fp32-packed": px * 3 * 4 + px * 4, "u8-u8": 2 * px * 3, "eager": 2 * px * 3}
    for n, ts in times.items():
        med = statistics.median(ts)
        print(json.dumps({"case": n, "shape": [B, T, 3, H, W], "metrics": ["psnr", "ssim", "msssim"],
                          "ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                          "blocks": args.blocks, "per_block": args.per_block,
                          "scale0_operand_bytes": read[n], "max_abs_diff_vs_eager": diff if n == "u8-u8" else None}))


if __name__ == "__main__":
    main()
