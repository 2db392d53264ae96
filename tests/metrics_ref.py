"""fp64 numpy restatement of the metrics the reference's scorer takes from TensorFlow (tools/eval/metrics.py:67-74:
tf.image.psnr / ssim / ssim_multiscale with max_val=1, TF's image_ops_impl.py), the yardstick of waldo_amd.metrics.
numpy only.  A frame is (H, W, 3) or (3, H, W) (``chw=True``) with values in [0, 1]."""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2  # (k1 max_val)^2, (k2 max_val)^2 with max_val=1 (metrics.py:68)
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # tf.image.ssim_multiscale's default (metrics.py:72)


def window(size=11, sigma=1.5):
    """TF's _fspecial_gauss: softmax of -0.5 (i - 5)^2 / sigma^2 over the 2-D grid = the outer product of this."""
    g = np.exp(-0.5 * (np.arange(size) - (size - 1) / 2.0) ** 2 / sigma ** 2)
    return g / g.sum()


def _corr_valid(x, g):
    """VALID correlation of (H, W) with g (x) g, separably: (H - k + 1, W - k + 1), no padding."""
    k = len(g)
    rows = np.lib.stride_tricks.sliding_window_view(x, k, axis=1) @ g
    return np.lib.stride_tricks.sliding_window_view(rows, k, axis=0) @ g


def ssim_channel(x, y):
    """(ssim_c, cs_c) of one (H, W) channel pair: TF's _ssim_per_channel / _ssim_helper (metrics.py:68, 72)."""
    g = window()
    mx, my = _corr_valid(x, g), _corr_valid(y, g)
    num0 = mx * my * 2.0
    den0 = mx * mx + my * my
    lum = (num0 + C1) / (den0 + C1)
    num1 = _corr_valid(x * y, g) * 2.0
    den1 = _corr_valid(x * x + y * y, g)
    cs = (num1 - num0 + C2) / (den1 - den0 + C2)
    return float(np.mean(lum * cs)), float(np.mean(cs))


def _hwc(a, chw):
    a = np.asarray(a, dtype=np.float64)
    return np.moveaxis(a, 0, -1) if chw else a


def ssim(a, b, chw=False):
    """tf.image.ssim (metrics.py:68): the mean over the channels of ssim_c."""
    a, b = _hwc(a, chw), _hwc(b, chw)
    return float(np.mean([ssim_channel(a[..., c], b[..., c])[0] for c in range(a.shape[-1])]))


def downscale(x):
    """One MS-SSIM scale step of an (H, W) channel: SYMMETRIC padding of an odd side by one row / column at the end,
    then the 2 x 2 average with stride 2 (tf.image.ssim_multiscale's do_pad + avg_pool, metrics.py:72)."""
    h, w = x.shape
    x = np.pad(x, ((0, h % 2), (0, w % 2)), mode="symmetric")
    return 0.25 * (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2])


def msssim(a, b, chw=False):
    """tf.image.ssim_multiscale (metrics.py:72): prod_k<4 relu(cs_k)^w_k * relu(ssim_4)^w_4 per channel, then the mean
    over the channels.  Raises ValueError when a scale falls below 11 x 11 (TF asserts it)."""
    a, b = _hwc(a, chw), _hwc(b, chw)
    vals = []
    for c in range(a.shape[-1]):
        x, y = a[..., c], b[..., c]
        prod = 1.0
        for k, wk in enumerate(MSSSIM_WEIGHTS):
            if k:
                x, y = downscale(x), downscale(y)
            if min(x.shape) < 11:
                raise ValueError(f"msssim: scale {k} is {x.shape[0]}x{x.shape[1]}, below 11x11")
            s, cs = ssim_channel(x, y)
            prod *= max(cs if k < len(MSSSIM_WEIGHTS) - 1 else s, 0.0) ** wk
        vals.append(prod)
    return float(np.mean(vals))


def psnr(a, b, chw=False):
    """tf.image.psnr (metrics.py:70): -10 log10(mse) over all pixels and channels; +inf for equal frames."""
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0.0 else -10.0 * np.log10(mse)


def quantize(x, span=(-1.0, 1.0), mode="trunc"):
    """The [0, 1] value frame_metrics scores for fp32 values: float32 operations as torch does them on the host."""
    lo, hi = span
    f = np.float32
    u = np.clip((np.asarray(x, f) - f(lo)) / f(hi - lo), f(0), f(1))
    if mode == "trunc":
        return np.trunc(u * f(255)) / f(255)
    if mode == "round":
        return np.trunc(u * f(255) + f(0.5)) / f(255)
    return u


def summarize(scores, vid_context):
    """metrics.py:95-113 on a dict name -> (clips, T): per t the mean / np.std over clips, and from vid_context on the
    mean / std over clips x frames vid_context..t."""
    out = {}
    for name, a in scores.items():
        a = np.asarray(a, np.float64)
        out[name] = {"per_t": [(float(a[:, t].mean()), float(a[:, t].std())) for t in range(a.shape[1])],
                     "cum": [(float(a[:, vid_context:t + 1].mean()), float(a[:, vid_context:t + 1].std()))
                             for t in range(vid_context, a.shape[1])]}
    return out
