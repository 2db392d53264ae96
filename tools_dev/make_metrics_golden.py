"""Writes tests/golden/metrics_skimage.npz: uint8 frame pairs and their SSIM / PSNR from scikit-image, the independent
check of tests/metrics_ref.py (tests/test_metrics_cpu.py).  scikit-image is no dependency of the library or of its tests:
run this once with an interpreter that has it (scikit-image 0.18), isolated from the repository's path, e.g.
``python -I tools_dev/make_metrics_golden.py``.  No test runs it."""
import os

import numpy as np
from skimage.metrics import peak_signal_noise_ratio, structural_similarity

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "metrics_skimage.npz")
SIZES = ((37, 53), (64, 96), (181, 243))  # odd and even; the last one >= 161 for MS-SSIM, odd: symmetric padding


def pair(rng, h, w):
    """A smooth frame with texture and a distorted copy of it (noise, a shift of brightness, a blurred region)."""
    coarse = rng.random((h // 8 + 2, w // 8 + 2, 3))
    smooth = np.kron(coarse, np.ones((8, 8, 1)))[:h, :w]
    a = np.clip(0.7 * smooth + 0.3 * rng.random((h, w, 3)), 0, 1)
    b = np.clip(a + 0.06 * rng.standard_normal(a.shape) + 0.03, 0, 1)
    b[: h // 3, : w // 3] = 0.5 * (b[: h // 3, : w // 3] + np.roll(b, 2, axis=1)[: h // 3, : w // 3])
    return (a * 255 + 0.5).astype(np.uint8), (b * 255 + 0.5).astype(np.uint8)


def main():
    rng = np.random.default_rng(2026)
    out = {}
    for i, (h, w) in enumerate(SIZES):
        a, b = pair(rng, h, w)
        fa, fb = a / 255.0, b / 255.0
        out[f"a{i}"], out[f"b{i}"] = a, b
        out[f"ssim{i}"] = np.float64(structural_similarity(fa, fb, gaussian_weights=True, sigma=1.5,
                                                           use_sample_covariance=False, data_range=1.0,
                                                           multichannel=True))
        out[f"psnr{i}"] = np.float64(peak_signal_noise_ratio(fa, fb, data_range=1.0))
        print(h, w, out[f"ssim{i}"], out[f"psnr{i}"])
    np.savez_compressed(OUT, n=np.int64(len(SIZES)), **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
