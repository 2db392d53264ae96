"""dev: tests/golden/augment_pil.npz -- two frames of the demo clip through the reference's RGB route
(data/base_dataset.py:330-370 with is_PIL=True: crop, Resize(BILINEAR), the two flips, ColorJitter, ToTensor), done
with PIL alone.

    python tools_dev/make_augment_golden.py

torchvision is not installed where this was written, so the reference's own ``get_transform`` could not be run: the PIL
calls below were written from knowledge of torchvision's PIL backend (``F.crop`` -> ``Image.crop``, ``Resize`` ->
``Image.resize((w, h), BILINEAR)``, ``adjust_brightness`` / ``adjust_saturation`` -> ``ImageEnhance.Brightness`` /
``ImageEnhance.Color``, ``adjust_hue`` -> ``convert("HSV")``, a wrapping uint8 add of ``hue * 255`` truncated toward zero
to the H channel, ``convert("RGB")``) and were NOT checked against torchvision.

Eight parameter draws at --colorjitter 0.5 / --max_zoom 1.3 (two of them without jitter) plus one that is resize only
(a fixed crop, no flip, no jitter), each applied to both frames at the output size 128 x 256.  Stored: the parameters,
the frames' names, and the bytes of the central REGION of every result (the whole result would not fit a committed
file)."""
import os
import random
import sys

import numpy as np
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from augment_ref import ORDERS, reference_parameters  # noqa: E402

FRAMES = os.path.join(ROOT, "tests", "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")
NAMES = ("munster_000037_000001_leftImg8bit.png", "munster_000037_000004_leftImg8bit.png")
OUT = os.path.join(ROOT, "tests", "golden", "augment_pil.npz")
SIZE = (128, 256)  # (H, W) of the result
REGION = (32, 64, 64, 128)  # top, left, height, width of the stored part
DRAWS = 8
NO_JITTER_DRAWS = (2, 5)


def adjust_hue(img, hue):
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.uint8(int(hue * 255) % 256)  # (uint8 arithmetic wraps)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_route(img, box, flip, jitter, order, size=SIZE):
    """The reference's RGB route on one PIL frame -> uint8 (H, W, 3); ``size`` the result's (H, W)."""
    top, left, hc, wc = box
    img = img.crop((left, top, left + wc, top + hc)).resize((size[1], size[0]), Image.BILINEAR)
    if flip & 1:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if flip & 2:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    if 0 <= order <= 5:
        for op in ORDERS[order]:
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(jitter[0])
            elif op == 1:
                img = ImageEnhance.Color(img).enhance(jitter[1])
            else:
                img = adjust_hue(img, jitter[2])
    return np.asarray(img, dtype=np.uint8)


def main():
    rng = random.Random(20240611)
    frames = [Image.open(os.path.join(FRAMES, n)).convert("RGB") for n in NAMES]
    h, w = frames[0].size[1], frames[0].size[0]
    box, flip, jitter, order, uniforms = [], [], [], [], []
    for d in range(DRAWS):
        u = [rng.random() for _ in range(8)]
        fl, bx, jt, _ = reference_parameters(u, h=h, w=w, aspect_ratio=2.0, true_ratio=2.0, max_zoom=1.3, lr_flip=True,
                                             tb_flip=True, colorjitter=0.5)
        uniforms.append(u)
        box.append(bx)
        flip.append(fl)
        jitter.append(jt)
        order.append([255] * len(NAMES) if d in NO_JITTER_DRAWS else [rng.randrange(6) for _ in NAMES])
    box.append([19, 37, 71, 142])  # resize only: non-dyadic ratios 71 -> 128 and 142 -> 256
    flip.append(0)
    jitter.append([1.0, 1.0, 0.0])
    order.append([255] * len(NAMES))
    t0, l0, rh, rw = REGION
    out = np.stack([np.stack([pil_route(frames[k], box[d], flip[d], jitter[d], order[d][k])[t0:t0 + rh, l0:l0 + rw]
                              for k in range(len(NAMES))]) for d in range(len(box))])
    np.savez_compressed(OUT, names=np.array(NAMES), size=np.array(SIZE, np.int32), region=np.array(REGION, np.int32),
                        uniforms=np.array(uniforms, np.float64), box=np.array(box, np.int32),
                        flip=np.array(flip, np.uint8), jitter=np.array(jitter, np.float32),
                        order=np.array(order, np.uint8), resize_only=np.array(len(box) - 1, np.int32), rgb=out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, rgb {out.shape}")


if __name__ == "__main__":
    main()
