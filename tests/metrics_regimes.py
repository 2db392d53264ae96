"""Operands for waldo_amd.metrics.frame_metrics chosen for their conditioning and their signs, the predicate that says
so, and fp32 restatements of the pass kernel's arithmetic (csrc/frame_metrics.hip).

The frames of tests/test_gpu_metrics.py are mid-grey and textured: the local variance is large against the local mean.
SSIM's variance term is a difference of two sums of about 2 mu^2, so a bright, nearly flat window (a saturated sky, a
white background reproduced up to a level or two) cancels most of their bits.  ``kappa`` measures that per window;
the builders below reach kappa of 2000, and the benign, the negative and the near-zero ``cs`` the MS-SSIM relu and its
powers meet.  Every builder is seeded and returns uint8 clips (B, T, 3, H, W) as torch tensors on the host.

``tf_order_fp32`` restates TF's ``_ssim_helper`` in fp32 in its operation order, which misses the bound on the bright
regimes; ``shifted_fp32`` restates the pass kernel's arithmetic: each 32 x 64 tile subtracts the mean of its staged
in-frame values from each operand, filters the differences, and adds the means back for the luminance only.
Both take the taps ascending, rows then columns, without fused multiply-add, and sum a thread's 8 outputs in fp32.
``fault=`` plants an error in them, for tests/test_metrics_regimes_cpu.py to show the criteria reject it.
numpy and torch on the CPU."""
import functools

import numpy as np
import torch

import metrics_ref as R
from test_gpu_metrics import TOL_PSNR, TOL_SSIM  # the project's bounds against fp64: 1e-4 dB, 1e-5

TILE_H, TILE_W, TAPS, ROWS_PER_THREAD = 32, 64, 11, 8  # csrc/frame_metrics.hip
SPAN = (-1.0, 1.0)
F = np.float32


def _rng(seed):
    return np.random.default_rng(seed)


def _u8(x):
    return torch.from_numpy(np.clip(np.rint(x), 0, 255).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------- builders
def textured(b, t, h, w, seed):
    """The operands of tests/test_gpu_metrics.py's ``_bytes``: a smooth clip with 30 % white noise and a 5 % distorted
    copy of it."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b * t, 3, h // 8 + 2, w // 8 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(coarse, scale_factor=8, mode="bilinear")[..., :h, :w]
    a = (0.7 * smooth + 0.3 * torch.rand(b * t, 3, h, w, generator=g)).clamp(0, 1)
    d = (a + 0.05 * torch.randn(a.shape, generator=g) + 0.02).clamp(0, 1)
    cvt = lambda x: (x * 255 + 0.5).to(torch.uint8).view(b, t, 3, h, w)  # noqa: E731
    return cvt(a), cvt(d)


def bright_flat(b, t, h, w, base, sd, seed):
    """Two independent draws of clip(round(base + N(0, sd)))."""
    g = _rng(seed)
    shape = (b, t, 3, h, w)
    return _u8(base + sd * g.standard_normal(shape)), _u8(base + sd * g.standard_normal(shape))


def flat_vs_noisy(b, t, h, w, base, sd, seed):
    """A constant frame against clip(round(base + N(0, sd)))."""
    shape = (b, t, 3, h, w)
    return _u8(np.full(shape, float(base))), _u8(base + sd * _rng(seed).standard_normal(shape))


def dark_flat(b, t, h, w, seed):
    """The benign counterpart of ``bright_flat``: a base of 0 ... 8 per (frame, channel), sd 1 -- flat, kappa small."""
    g = _rng(seed)
    shape = (b, t, 3, h, w)
    base = g.integers(0, 9, size=(b, t, 3, 1, 1)).astype(np.float64)
    return _u8(base + g.standard_normal(shape)), _u8(base + g.standard_normal(shape))


def mixed_tile(b, t, h, w, seed):
    """Within every 32 x 64 tile the left half is bright and flat (255 + N(0, 1), drawn twice) and the right half is
    textured with mean about 80, where the second frame equals the first up to +-6 levels: no single constant per
    tile is near both halves."""
    g = _rng(seed)
    shape = (b, t, 3, h, w)
    tex = 80.0 + 60.0 * (g.random(shape) - 0.5) + 20.0 * np.sin(np.arange(w) * 0.9)[None, None, None, None, :]
    left = (np.arange(w) % TILE_W) < TILE_W // 2
    a = np.where(left, 255.0 + g.standard_normal(shape), tex)
    d = np.where(left, 255.0 + g.standard_normal(shape), np.rint(tex) + g.integers(-6, 7, size=shape))
    return _u8(a), _u8(d)


def inverted(b, t, h, w, seed):
    """White noise and 255 minus it: every window's covariance, so every ``cs`` of the full scale, is negative."""
    a = _rng(seed).integers(0, 256, size=(b, t, 3, h, w)).astype(np.uint8)
    return torch.from_numpy(a), torch.from_numpy(255 - a)


def _blend(a, lam, noise):
    return np.clip(np.rint(lam * a + (1.0 - lam) * (255.0 - a) + noise), 0, 255)


def near_zero_cs(b, t, h, w, seed):
    """White noise a against lam a + (1 - lam) (255 - a) + N(0, 4): lam 0.45 in channel 0 (mean cs at scale 0
    negative), 0.55 in channel 1 (positive), and in channel 2 the lam found by bisection, per frame, at which the
    fp64 mean cs at scale 0 is within 1e-3 of zero."""
    g = _rng(seed)
    a = g.integers(0, 256, size=(b, t, 3, h, w)).astype(np.float64)
    noise = 4.0 * g.standard_normal(a.shape)
    d = np.empty_like(a)
    for i in range(b):
        for j in range(t):
            d[i, j, 0] = _blend(a[i, j, 0], 0.45, noise[i, j, 0])
            d[i, j, 1] = _blend(a[i, j, 1], 0.55, noise[i, j, 1])
            x, n = a[i, j, 2], noise[i, j, 2]
            cs = lambda lam: R.ssim_channel(x / 255.0, _blend(x, lam, n) / 255.0)[1]  # noqa: E731
            lo, hi = 0.45, 0.55  # cs(lo) < 0 < cs(hi)
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                v = cs(mid)
                if abs(v) < 2e-4:
                    break
                lo, hi = (mid, hi) if v < 0 else (lo, mid)
            d[i, j, 2] = _blend(x, mid, n)
    return torch.from_numpy(a.astype(np.uint8)), torch.from_numpy(d.astype(np.uint8))


def single_pixel(b, t, h, w, seed, frame=(0, 0)):
    """Equal textured frames, except that one pixel of one channel of frame ``frame`` differs by one level.  Returns
    (a, d, (channel, y, x))."""
    g = _rng(seed)
    a = textured(b, t, h, w, seed)[0]
    d = a.clone()
    c, y, x = int(g.integers(0, 3)), int(g.integers(0, h)), int(g.integers(0, w))
    v = int(a[frame[0], frame[1], c, y, x])
    d[frame[0], frame[1], c, y, x] = v + 1 if v < 255 else v - 1
    return a, d, (c, y, x)


def as_fp32(u8, seed, span=SPAN):
    """An fp32 clip in ``span`` whose [0, 1] values sit at the bytes plus a uniform jitter of +-0.4 level: under
    ``quantize="none"`` the operand is not byte-quantised (and the kernel's 256-entry table is not used)."""
    g = torch.Generator().manual_seed(seed)
    jit = (torch.rand(u8.shape, generator=g) - 0.5) * 0.8
    lo, hi = span
    return (lo + (u8.float() + jit) / 255.0 * (hi - lo)).float()


# the conditioning regimes tests/test_gpu_metrics_regimes.py runs through every encoding: name -> builder(b, t, h, w)
BRIGHT = ("bright255_sd1", "bright250_sd1", "bright235_sd1", "bright250_sd2", "flat240_vs_sd3")
REGIMES = {
    "bright255_sd1": lambda *s: bright_flat(*s, 255, 1, seed=0),
    "bright250_sd1": lambda *s: bright_flat(*s, 250, 1, seed=1),
    "bright235_sd1": lambda *s: bright_flat(*s, 235, 1, seed=2),
    "bright250_sd2": lambda *s: bright_flat(*s, 250, 2, seed=3),
    "flat240_vs_sd3": lambda *s: flat_vs_noisy(*s, 240, 3, seed=4),
    "dark_flat": lambda *s: dark_flat(*s, seed=5),
    "mixed_tile": lambda *s: mixed_tile(*s, seed=6),
    "inverted": lambda *s: inverted(*s, seed=7),
    "near_zero_cs": lambda *s: near_zero_cs(*s, seed=8),
    "single_pixel": lambda *s: single_pixel(*s, seed=9)[:2],
}
SSIM_HW, MS_HW = (75, 139), (161, 193)  # 161 = 5 * 32 + 1, 193 = 3 * 64 + 1: odd at every scale down to 11 x 13


@functools.lru_cache(maxsize=None)
def regime(name, b, t, h, w):
    """The two uint8 clips of a regime, built once per shape; do not write to them."""
    return REGIMES[name](b, t, h, w)


# --------------------------------------------------------------------------------------------------------- predicate
def kappa(x, y):
    """(mu_x^2 + mu_y^2) / (sigma_x^2 + sigma_y^2 + C2) of every 11 x 11 window of an (H, W) channel pair in [0, 1],
    from the fp64 restatement: how many times larger the two sums the variance term subtracts are than the term."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    g = R.window()
    mx, my = R._corr_valid(x, g), R._corr_valid(y, g)
    den0 = mx * mx + my * my
    return den0 / (R._corr_valid(x * x + y * y, g) - den0 + R.C2)


def median_kappa(a, d):
    """Median kappa over the frames and channels of two uint8 clips."""
    a, d = a.numpy().reshape(-1, *a.shape[-2:]) / 255.0, d.numpy().reshape(-1, *d.shape[-2:]) / 255.0
    return float(np.median(np.concatenate([kappa(p, q).ravel() for p, q in zip(a, d)])))


# ------------------------------------------------------------------------------------------------- fp32 restatements
def _window32(fault=None):
    i = np.arange(TAPS)
    g = np.exp(-0.5 * (i - 5.0) ** 2 / 1.5 ** 2)
    if fault == "centre_tap":
        g[5] += 1e-3
    return (g / g.sum()).astype(F)


def _taps(v, g, axis):
    """The 11-tap correlation of fp32 ``v`` along ``axis``, taps ascending from 0.0f, a multiply and an add per tap."""
    n = v.shape[axis] - TAPS + 1
    acc = np.zeros([n if k == axis else s for k, s in enumerate(v.shape)], F)
    for j in range(TAPS):
        acc = acc + g[j] * np.take(v, range(j, j + n), axis=axis)
    return acc


def _channel32(x, y, shift, fault=None):
    """(sum lum * cs, sum cs, VALID outputs) of one fp32 (H, W) channel pair, tile by tile as the pass kernel."""
    h, w = x.shape
    g = _window32(fault)
    c1, c2 = F(0.01) * F(0.01), F(0.03) * F(0.03)
    if fault == "c2":
        c2 = F(c2 * F(1.01))
    hv, wv = h - TAPS + 1, w - TAPS + 1
    rows = hv + 1 if fault == "valid_row" else hv
    s_ssim = s_cs = 0.0
    for y0 in range(0, h, TILE_H):
        for x0 in range(0, w, TILE_W):
            sx = np.zeros((TILE_H + TAPS - 1, TILE_W + TAPS - 1), F)
            sy = np.zeros_like(sx)
            ph, pw = min(h - y0, sx.shape[0]), min(w - x0, sx.shape[1])
            sx[:ph, :pw] = x[y0:y0 + ph, x0:x0 + pw]
            sy[:ph, :pw] = y[y0:y0 + ph, x0:x0 + pw]
            cx = cy = F(0)
            if shift:
                cx, cy = sx[:ph, :pw].mean(dtype=F), sy[:ph, :pw].mean(dtype=F)
            dx, dy = sx - cx, sy - cy
            e = [_taps(_taps(q, g, 1), g, 0) for q in (dx, dy, dx * dx + dy * dy, dx * dy)]
            mx, my = e[0] + cx, e[1] + cy
            lum = (mx * my * F(2) + c1) / (mx * mx + my * my + c1)
            cs = (e[3] * F(2) - e[0] * e[1] * F(2) + c2) / (e[2] - (e[0] * e[0] + e[1] * e[1]) + c2)
            ok = ((y0 + np.arange(TILE_H))[:, None] < rows) & ((x0 + np.arange(TILE_W))[None, :] < wv)
            for q, m in ((0, lum * cs), (1, cs)):
                m = np.where(ok, m, F(0)).reshape(TILE_H // ROWS_PER_THREAD, ROWS_PER_THREAD, TILE_W)
                acc = np.zeros((m.shape[0], TILE_W), F)
                for o in range(ROWS_PER_THREAD):  # a thread's 8 outputs, in fp32
                    acc = acc + m[:, o]
                if q == 0:
                    s_ssim += float(acc.astype(np.float64).sum())
                else:
                    s_cs += float(acc.astype(np.float64).sum())
    return s_ssim, s_cs, hv * wv


def _pool32(x, fault=None):
    """The next scale of an fp32 (H, W) channel: ((a + b) + (c + d)) * 0.25, the last row / column again at an odd
    end."""
    h, w = x.shape
    mode = "constant" if fault == "zero_pad" else "symmetric"
    x = np.pad(x, ((0, h % 2), (0, w % 2)), mode=mode)
    return ((x[0::2, 0::2] + x[0::2, 1::2]) + (x[1::2, 0::2] + x[1::2, 1::2])) * F(0.25)


def _ssim32(a, d, shift, fault):
    a, d = np.asarray(a, F), np.asarray(d, F)
    tot = 0.0
    for c in range(3):
        s, _, n = _channel32(a[c], d[c], shift, fault)
        tot += s / n
    return float(F(tot / 3.0))


def _msssim32(a, d, shift, fault):
    a, d = np.asarray(a, F), np.asarray(d, F)
    tot = 0.0
    for c in range(3):
        x, y = a[c], d[c]
        prod = 1.0
        for k, wk in enumerate(R.MSSSIM_WEIGHTS):
            if k:
                x, y = _pool32(x, fault), _pool32(y, fault)
            s, cs, n = _channel32(x, y, shift, fault)
            v = (cs if k < len(R.MSSSIM_WEIGHTS) - 1 else s) / n
            with np.errstate(invalid="ignore"):  # without the relu a negative mean gives nan, as pow() does
                prod *= float(np.power(v if fault == "no_relu" else max(v, 0.0), wk))
        tot += prod
    return float(F(tot / 3.0))


def tf_order_fp32(a, d, fault=None):
    """SSIM of two (3, H, W) frames in [0, 1]: fp32, TF's ``_ssim_helper`` in its operation order."""
    return _ssim32(a, d, False, fault)


def tf_order_fp32_ms(a, d, fault=None):
    """MS-SSIM of two (3, H, W) frames in [0, 1]: ``tf_order_fp32`` at every scale, fp32 pooling."""
    return _msssim32(a, d, False, fault)


def shifted_fp32(a, d, fault=None):
    """SSIM as the pass kernel computes it: the operands shifted by their tile's means."""
    return _ssim32(a, d, True, fault)


def shifted_fp32_ms(a, d, fault=None):
    return _msssim32(a, d, True, fault)


def psnr_fp32(a, d, fault=None):
    """PSNR of two (3, H, W) frames in [0, 1] as the kernels sum it: fp32 differences and squares, summed in fp64 over
    each tile's own pixels.  ``fault="apron_se"`` sums over the tile's 10-pixel apron as well."""
    a, d = np.asarray(a, F), np.asarray(d, F)
    _, h, w = a.shape
    ext = TAPS - 1 if fault == "apron_se" else 0
    se = 0.0
    for y0 in range(0, h, TILE_H):
        for x0 in range(0, w, TILE_W):
            e = a[:, y0:y0 + TILE_H + ext, x0:x0 + TILE_W + ext] - d[:, y0:y0 + TILE_H + ext, x0:x0 + TILE_W + ext]
            se += float((e * e).astype(np.float64).sum())
    mse = se / (3.0 * h * w)
    return float("inf") if mse == 0.0 else float(F(-10.0 * np.log10(mse)))


# ---------------------------------------------------------------------------------------------------------- criteria
def unit(u8):
    """The fp32 [0, 1] frames of a uint8 clip, as the kernel's table holds them."""
    return u8.numpy().astype(F) / F(255)


def reference(p, r, metrics):
    """The fp64 restatement's (B, T) scores of the [0, 1] clips ``p``, ``r`` ((B, T, 3, H, W) numpy)."""
    fn = {"psnr": R.psnr, "ssim": lambda x, y: R.ssim(x, y, chw=True), "msssim": lambda x, y: R.msssim(x, y, chw=True)}
    return {m: np.array([[fn[m](p[i, j], r[i, j]) for j in range(p.shape[1])] for i in range(p.shape[0])])
            for m in metrics}


def fractions(got, ref):
    """The criterion of every comparison here and in tests/test_gpu_metrics_regimes.py: per metric of ``ref`` the
    largest |got - ref| over the frames as a fraction of the metric's bound, TOL_PSNR or TOL_SSIM; an infinite
    reference (PSNR of equal frames) must be met exactly, and a nan counts as inf."""
    out = {}
    for m, want in ref.items():
        have = np.asarray(got[m], np.float64)
        assert have.shape == want.shape, (m, have.shape, want.shape)
        with np.errstate(invalid="ignore"):
            frac = np.abs(have - want) / (TOL_PSNR if m == "psnr" else TOL_SSIM)
        frac = np.where(np.isinf(want) | np.isinf(have), np.where(have == want, 0.0, np.inf), frac)
        out[m] = float(np.where(np.isnan(frac), np.inf, frac).max())
    return out


def restated(p, r, metrics, shift=True, fault=None):
    """``got`` of ``fractions`` from the fp32 restatements instead of the kernel."""
    fn = {"psnr": lambda x, y: psnr_fp32(x, y, fault), "ssim": lambda x, y: _ssim32(x, y, shift, fault),
          "msssim": lambda x, y: _msssim32(x, y, shift, fault)}
    return {m: [[fn[m](p[i, j], r[i, j]) for j in range(p.shape[1])] for i in range(p.shape[0])] for m in metrics}
