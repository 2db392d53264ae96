"""Writes tests/golden/render_reference.npz: what the reference's own ``Logger.get_lyt`` and ``Logger.get_flow_rgb``
(tools/logger.py:169-179, 310-318) return for small seeded inputs, the colour tables matplotlib holds for them and the
reference's two dataset palettes -- the fixture of tests/test_render_abi.py and tests/test_gpu_render.py.  Data only.

    python tools_dev/make_render_golden.py [REFERENCE_ROOT]

Needs the reference tree (default /root/reference, or $WALDO_REFERENCE_ROOT) and matplotlib; no test runs it.  The
reference's two files are executed from where they lie, under stand-ins used when torchvision / tensorboard are not
installed or matplotlib is 3.9 or later:
  * ``torch.utils.tensorboard`` (only ``Logger.__init__`` uses it; the Logger here is made with ``Logger.__new__``);
  * ``torchvision``: ``transforms.Compose`` / ``ToTensor`` / ``Normalize`` written below from their documented semantics
    (``color_transfer`` sends every frame through them), the rest as empty names;
  * ``matplotlib.cm.get_cmap(name, lut)``, removed in matplotlib 3.9: ``matplotlib.colormaps[name].resampled(lut)``, which
    is what it returned.
(The loading is done here and not through the test suite's reference-import harness: development scripts stay clear of
that package -- tests/test_abi.py.)"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "render_reference.npz")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WALDO_REFERENCE_ROOT", "/root/reference")
TABLE_SIZES = (4, 8, 12, 17, 20)
LAYERS = (4, 17)


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class ToTensor:
    """A PIL image (H, W, C) of bytes -> a float tensor (C, H, W) in [0, 1]: byte / 255."""

    def __call__(self, pic):
        a = np.asarray(pic)
        a = a[:, :, None] if a.ndim == 2 else a
        return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class Normalize:
    """(x - mean) / std per channel."""

    def __init__(self, mean, std):
        self.mean, self.std = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)

    def __call__(self, x):
        return (x - self.mean) / self.std


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def _load(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


def load_logger():
    """The reference's Logger class, with the stand-ins of the module docstring in place."""
    import matplotlib
    from matplotlib import cm
    sys.dont_write_bytecode = True
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = lambda name, lut=None: matplotlib.colormaps[name] if lut is None else matplotlib.colormaps[name].resampled(lut)
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms", Compose=Compose, ToTensor=ToTensor, Normalize=Normalize,
                          GaussianBlur=object)
    tv.utils = _stub("torchvision.utils", make_grid=None)
    tv.io = _stub("torchvision.io")
    tv.models = _stub("torchvision.models")
    try:
        import torch.utils.tensorboard  # noqa: F401
    except Exception:
        _stub("torch.utils.tensorboard", SummaryWriter=object)
    tools = _stub("tools")
    tools.__path__ = [os.path.join(REF, "tools")]
    tools.utils = _load("tools.utils", "tools/utils.py")
    return _load("tools.logger", "tools/logger.py").Logger


def option_palettes():
    """The two palette lists of the reference's option defaults (tools/options.py), read as data."""
    tree = ast.parse(open(os.path.join(REF, "tools", "options.py")).read())
    found = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id in ("CITYSCAPES_PALETTE", "KITTI_PALETTE"):
            found[node.targets[0].id] = [int(v) for v in ast.literal_eval(node.value)]
    return found["CITYSCAPES_PALETTE"], found["KITTI_PALETTE"]


def coarse(rng, shape):
    """Seeded fp32 values on a grid of 1 / 16 (exact in bf16 and fp16 too; equal maxima occur on their own)."""
    return (np.round(rng.standard_normal(shape) * 24) / 16).astype(np.float32)


def plant_ties(x):
    """An all-equal pixel, two equal maxima (the lower channel must win), and one where the LAST channels tie."""
    c = x.shape[2]
    x[0, 0, :, 0, 0] = 0.25
    if c > 2:
        x[0, 1, :, 3, 5] = -1.0
        x[0, 1, 1, 3, 5] = x[0, 1, c - 1, 3, 5] = 7.0
        x[1, 2, :, 11, 19] = 0.0
        x[1, 2, c - 2, 11, 19] = x[1, 2, c - 1, 11, 19] = 3.5
    return x


def main():
    import matplotlib
    Logger = load_logger()
    city, kitti = option_palettes()
    rng = np.random.default_rng(20261018)
    out = {"palette_cityscapes": np.array(city, dtype=np.int64), "palette_kitti": np.array(kitti, dtype=np.int64)}

    def logger_with(palette, num_lyt):  # what Logger.__init__ derives from the options (tools/logger.py:16-18), by its rule
        lg = Logger.__new__(Logger)
        if palette is not None:
            lg.palette = np.array([palette[3 * k: 3 * (k + 1)] + [255] for k in range(num_lyt)]).astype(np.float64) / 255
        return lg

    plain = logger_with(None, 0)
    logits = plant_ties(coarse(rng, (2, 3, 20, 12, 20)))
    out["logits"] = logits
    out["lyt_jet20"] = plain.get_lyt(torch.from_numpy(logits), 20, use_palette=False).numpy()
    assert len(city) == 60 and len(kitti) == 57
    out["lyt_cityscapes"] = logger_with(city, 20).get_lyt(torch.from_numpy(logits), 20, use_palette=True).numpy()
    out["lyt_kitti"] = logger_with(kitti, 19).get_lyt(torch.from_numpy(logits[:, :, :19].copy()), 19,
                                                     use_palette=True).numpy()
    for L in LAYERS:
        alpha = plant_ties(coarse(rng, (2, 3, L, 12, 20)))
        out[f"alpha{L}"] = alpha
        out[f"lyt_alpha{L}"] = plain.get_lyt(torch.from_numpy(alpha), L, use_palette=False).numpy()

    flow = np.empty((3, 24, 40, 2), dtype=np.float32)
    flow[0] = rng.standard_normal((24, 40, 2)) * 0.05
    flow[1] = rng.standard_normal((24, 40, 2)) * 0.15  # (r reaches its clamp)
    flow[2] = rng.standard_normal((24, 40, 2)) * 0.05
    # planted: 32 pixels (1.1 % of the fixture), every one ON a boundary between two bins of the wheel
    flow[2, 0, :8] = 0.0                                # zeros
    flow[2, 1, :8, 1] = 0.0                             # along +u / -u
    flow[2, 2, :8, 0] = 0.0                             # along +v / -v
    flow[2, 3, :8, 0] = np.abs(flow[2, 3, :8, 0])
    flow[2, 3, :8, 1] = flow[2, 3, :8, 0]               # the diagonal
    out["flow"] = flow
    out["flow_rgb"] = plain.get_flow_rgb(torch.from_numpy(flow), mul=10).numpy()

    for n in TABLE_SIZES:
        out[f"jet{n + 1}"] = np.asarray(matplotlib.cm.get_cmap("jet", n + 1)(np.arange(n + 1))[:, :3], dtype=np.float64)
    out["hsv128"] = np.asarray(matplotlib.cm.get_cmap("hsv", 128)(np.arange(128))[:, :3], dtype=np.float64)

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    for k, v in out.items():
        print(f"  {k}: {v.dtype} {v.shape}")


if __name__ == "__main__":
    main()
