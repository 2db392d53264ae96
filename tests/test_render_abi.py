"""CPU: the C ABI and the Python surface of the renders (include/waldo_hip.h "Renders": waldo_render_argmax_fwd,
waldo_render_flow_fwd; waldo_amd.render).  No kernel is launched and no GPU is touched: every check here is argument
validation on the host, or the host-side colour tables against the fixture recorded from the reference
(tests/golden/render_reference.npz, tools_dev/make_render_golden.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_reference.npz")

F32, F16, BF16, PACKED = 0, 1, 2, 3
NCHW, NHWC = 0, 1
TRUNC, ROUND, NONE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def amax(lib, src=4, code=F32, ss=(320, 16, 4), palette=1, ids=1, di_n=16, rgb=1, dr_n=48, layout=NCHW, n=1, c=20, h=4,
         w=4):
    """waldo_render_argmax_fwd with one argument off; the pointers are never dereferenced (every case is refused, or
    returns, before a launch)."""
    return lib.waldo_render_argmax_fwd(src, code, *ss, palette, ids, di_n, rgb, dr_n, layout, n, c, h, w, None)


def flw(lib, flow=4, code=F32, ss=(32, 16, 4), wheel=4, k=128, mul=10.0, rgb=1, dr_n=48, layout=NCHW, quant=TRUNC, n=1,
        h=4, w=4):
    return lib.waldo_render_flow_fwd(flow, code, *ss, wheel, k, mul, rgb, dr_n, layout, quant, n, h, w, None)


def test_symbols_are_exported_and_bound(lib):
    from waldo_amd import _lib
    for name in ("waldo_render_argmax_fwd", "waldo_render_flow_fwd"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][-1] is ctypes.c_void_p
        assert len(_lib.SIGNATURES[name]) == 16
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Renders:"):]
    for needle in ("waldo_render_argmax_fwd", "waldo_render_flow_fwd", "v > best || (v != v && best == best)",
                   "atan2f(v, u)", "rgb[pixel] = palette[id]", "NaN in u or v gives bytes 0"):
        assert needle in sec, needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


@pytest.mark.parametrize("kw,msg", [
    (dict(code=PACKED), b"unknown dtype"), (dict(code=4), b"unknown dtype"), (dict(code=-1), b"unknown dtype"),
    (dict(layout=2), b"unknown layout"), (dict(layout=-1), b"unknown layout"),
    (dict(ss=(-320, 16, 4)), b"negative stride"), (dict(ss=(320, -16, 4)), b"negative stride"),
    (dict(ss=(320, 16, -4)), b"negative stride"), (dict(di_n=-16), b"negative stride"), (dict(dr_n=-48), b"negative stride"),
    (dict(n=-1), b"bad shape"), (dict(c=0), b"bad shape"), (dict(c=257), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(w=0), b"bad shape"), (dict(h=32769), b"bad shape"), (dict(w=32769), b"bad shape"),
    (dict(src=None), b"null pointer"), (dict(ids=None, rgb=None), b"null pointer"), (dict(palette=None), b"null pointer"),
    (dict(src=2), b"not aligned"), (dict(src=6), b"not aligned"), (dict(code=F16, src=1), b"not aligned"),
    (dict(code=BF16, src=3), b"not aligned"),
    (dict(n=2 ** 31), b"too large"),                    # one workgroup per frame: a grid of 2^31
    (dict(n=2 ** 40, h=32768, w=32768), b"too large"),
])
def test_argmax_rejects_bad_arguments(lib, kw, msg):
    assert amax(lib, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


def test_argmax_accepts_either_output_alone_up_to_the_launch(lib):
    """ids without a palette and rgb without ids are valid argument sets: with N == 0 they return before any launch."""
    assert amax(lib, n=0, src=None, ids=None, rgb=None, palette=None) == 0
    assert amax(lib, n=0, src=None, ids=None, rgb=None, palette=None, code=BF16, layout=NHWC, c=256) == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(code=PACKED), b"unknown dtype"), (dict(code=-1), b"unknown dtype"),
    (dict(layout=2), b"unknown layout"),
    (dict(quant=NONE), b"unknown quantisation"), (dict(quant=-1), b"unknown quantisation"),
    (dict(mul=float("nan")), b"bad multiplier"), (dict(mul=float("inf")), b"bad multiplier"),
    (dict(mul=float("-inf")), b"bad multiplier"),
    (dict(k=0), b"bad shape"), (dict(k=-3), b"bad shape"), (dict(k=4097), b"bad shape"), (dict(n=-1), b"bad shape"),
    (dict(h=0), b"bad shape"), (dict(w=32769), b"bad shape"),
    (dict(ss=(-32, 16, 4)), b"negative stride"), (dict(ss=(32, -16, 4)), b"negative stride"),
    (dict(ss=(32, 16, -4)), b"negative stride"), (dict(dr_n=-1), b"negative stride"),
    (dict(flow=None), b"null pointer"), (dict(wheel=None), b"null pointer"), (dict(rgb=None), b"null pointer"),
    (dict(flow=2), b"not aligned"), (dict(code=F16, flow=1), b"not aligned"),
    (dict(n=2 ** 31), b"too large"),
])
def test_flow_rejects_bad_arguments(lib, kw, msg):
    assert flw(lib, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


def test_empty_batch_returns_ok_without_a_launch(lib):
    assert flw(lib, n=0, flow=None, wheel=None, rgb=None) == 0
    assert flw(lib, n=0, flow=None, wheel=None, rgb=None, code=F16, layout=NHWC, quant=ROUND) == 0


# ---------------------------------------------------------------------------------------------------------------------
# host tables
# ---------------------------------------------------------------------------------------------------------------------
TABLE_SIZES = (4, 8, 12, 17, 20)


def test_colormap_tables_equal_the_fixture_bit_for_bit(golden):
    from waldo_amd import render as R
    for n in TABLE_SIZES:
        assert np.array_equal(R.colormap_table("jet", n + 1), golden[f"jet{n + 1}"]), n
    assert np.array_equal(R.colormap_table("hsv", 128), golden["hsv128"])
    wheel = R.flow_wheel(128)
    assert wheel.dtype == np.float32 and wheel.shape == (128, 3)
    assert np.array_equal(wheel, golden["hsv128"].astype(np.float32))
    assert np.array_equal(R.flow_wheel(), wheel)


def test_layer_palette_is_the_references_truncated_jet(golden):
    from waldo_amd import render as R
    for n in TABLE_SIZES:
        table = golden[f"jet{n + 1}"]
        cmap = table[(np.linspace(0, 1, n + 1)[:n] * (n + 1)).astype(int)].copy()
        cmap[0] = 0.5
        pal = R.layer_palette(n)
        assert pal.dtype == np.uint8 and pal.shape == (n, 3)
        assert np.array_equal(pal, (255 * cmap).astype(np.uint8)), n
    assert R.layer_palette(12)[:4].tolist() == [[127, 127, 127], [0, 0, 224], [0, 42, 255], [0, 127, 255]]


def _bytes_of(lyt):
    """get_lyt's values (ToTensor, then Normalize(0.5, 0.5): (byte / 255 - 0.5) / 0.5) mapped back to the bytes."""
    return np.round((lyt.astype(np.float64) * 0.5 + 0.5) * 255).astype(np.uint8)


def test_palettes_reproduce_get_lyt_of_the_fixture(golden):
    """Host side of the RGB check: palette[torch.max's index] equals what the reference's get_lyt returned."""
    from waldo_amd import render as R

    def render(x, pal):
        ids = torch.from_numpy(x).max(dim=-3)[1].numpy()
        return np.moveaxis(pal[ids], -1, -3)

    for L in (4, 17):
        assert np.array_equal(render(golden[f"alpha{L}"], R.layer_palette(L)), _bytes_of(golden[f"lyt_alpha{L}"])), L
    logits = golden["logits"]
    assert np.array_equal(render(logits, R.layer_palette(20)), _bytes_of(golden["lyt_jet20"]))
    city, kitti = R.semantic_palette(golden["palette_cityscapes"]), R.semantic_palette(golden["palette_kitti"])
    assert city.shape == (20, 3) and kitti.shape == (19, 3)
    assert np.array_equal(render(logits, city), _bytes_of(golden["lyt_cityscapes"]))
    assert np.array_equal(render(logits[:, :, :19], kitti), _bytes_of(golden["lyt_kitti"]))


def test_semantic_palette_is_the_float64_round_trip():
    from waldo_amd import render as R
    p = np.arange(256).repeat(3)
    want = (255 * (p.reshape(-1, 3).astype(np.float64) / 255)).astype(np.uint8)
    assert np.array_equal(R.semantic_palette(p.tolist()), want)
    assert np.all(want.ravel().astype(int) - p <= 0) and np.all(p - want.ravel().astype(int) <= 1)
    with pytest.raises(ValueError):
        R.semantic_palette([1, 2, 3, 4])
    with pytest.raises(ValueError):
        R.semantic_palette([1, 2, 256])


def test_tables_equal_matplotlib_where_it_is_installed():
    matplotlib = pytest.importorskip("matplotlib")
    from waldo_amd import render as R
    for name, sizes in (("jet", (1, 2, 5, 9, 13, 18, 21, 33, 257)), ("hsv", (1, 2, 7, 128, 256, 4096))):
        for n in sizes:
            want = matplotlib.colormaps[name].resampled(n)(np.arange(n))[:, :3]
            assert np.array_equal(R.colormap_table(name, n), want), (name, n)
    for n in (1, 2, 3, 12, 33, 256):  # a colormap called with floats: entry int(x * N)
        cmap = matplotlib.colormaps["jet"].resampled(n + 1)(np.linspace(0, 1, n + 1)[:n])
        cmap[0, :3] = 0.5
        assert np.array_equal(R.layer_palette(n), (255 * cmap[:, :3]).astype(np.uint8)), n


def test_the_product_does_not_import_matplotlib():
    text = open(os.path.join(ROOT, "waldo_amd", "render.py")).read()
    assert "import matplotlib" not in text and "from matplotlib" not in text


# ---------------------------------------------------------------------------------------------------------------------
# Python-side errors
# ---------------------------------------------------------------------------------------------------------------------
def test_wrappers_have_no_cpu_fallback():
    from waldo_amd import render as R
    from waldo_amd._lib import WaldoHipError
    x = torch.zeros(2, 4, 6, 8)
    with pytest.raises(WaldoHipError):
        R.class_ids(x)
    with pytest.raises(WaldoHipError):
        R.render_argmax(x, R.layer_palette(4))
    with pytest.raises(WaldoHipError):
        R.render_argmax(x, R.layer_palette(4), layout="nhwc", return_ids=True)
    with pytest.raises(WaldoHipError):
        R.render_flow(torch.zeros(2, 2, 6, 8))


def test_wrappers_refuse_bad_shapes_and_names():
    from waldo_amd import render as R
    x = torch.zeros(2, 4, 6, 8)
    with pytest.raises(ValueError, match="C = 257"):
        R.class_ids(torch.zeros(1, 257, 2, 2))
    with pytest.raises(ValueError, match="3 rows for C = 4"):
        R.render_argmax(x, R.layer_palette(3))
    with pytest.raises(ValueError, match="out must be a uint8 tensor of shape"):
        R.render_argmax(x, R.layer_palette(4), layout="nhwc", out=torch.zeros(2, 3, 6, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be a uint8 tensor of shape"):
        R.render_flow(torch.zeros(2, 2, 6, 8), layout="nhwc", out=torch.zeros(2, 3, 6, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="layout"):
        R.render_argmax(x, R.layer_palette(4), layout="hwc")
    with pytest.raises(ValueError, match="quantize"):
        R.render_flow(torch.zeros(2, 2, 6, 8), quantize="none")
    with pytest.raises(ValueError, match="2 channels"):
        R.render_flow(torch.zeros(2, 3, 6, 8))
    with pytest.raises(ValueError, match="mul"):
        R.render_flow(torch.zeros(2, 2, 6, 8), mul=float("inf"))
    with pytest.raises(ValueError):
        R.class_ids(torch.zeros(2, 4, 6, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        R.class_ids(torch.zeros(6, 8))
    with pytest.raises(ValueError, match="palette"):
        R.render_argmax(x, None)
    with pytest.raises(ValueError, match="bytes"):
        R.render_argmax(x, np.full((4, 3), 300))
    with pytest.raises(ValueError):
        R.layer_palette(0)
    with pytest.raises(ValueError):
        R.flow_wheel(4097)


def test_predict_refuses_an_unknown_render_and_units_to_clips_shapes_the_render_keys():
    """Host logic of tools.demo around the renders: the argument check, and the ranks' unit blocks of the new keys put
    back into predict()'s shapes (the reconstruction's units from dealing order to frame order)."""
    from waldo_amd.tools import demo
    with pytest.raises(ValueError, match="render"):
        demo.predict(None, None, None, torch.zeros(1, 6, 3, 4, 4), None, None, 4, render="floor")
    with pytest.raises(ValueError, match="render"):
        demo.predict_sharded(demo.demo_opt(dim=16), None, None, torch.zeros(1, 6, 3, 4, 4), None, None, 4, 0, 2,
                             render="floor")
    b, t, ctx, world, h, w = 2, 6, 4, 3, 4, 8
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 20, (b, t, h, w), generator=g, dtype=torch.uint8)
    order = [i for r in range(world) for i in demo.local_unit_ids("rec", b, t, ctx, r, world)]
    dealt = ids.view(b * t, 1, h, w)[order]
    assert torch.equal(demo.units_to_clips("rec_lyt_ids", dealt, b, t, ctx, world), ids)
    sem = torch.randint(0, 256, (b, t - ctx, 3, h, w), generator=g, dtype=torch.uint8)
    assert torch.equal(demo.units_to_clips("pred_sem_lyt", sem.view(-1, 3, h, w), b, t, ctx, world), sem)
    pic = torch.randint(0, 256, (b, ctx, t - ctx, 3, h, w), generator=g, dtype=torch.uint8)
    units = pic.permute(0, 2, 1, 3, 4, 5).reshape(b * (t - ctx), ctx * 3, h, w)
    assert torch.equal(demo.units_to_clips("pred_flow_rgb", units, b, t, ctx, world), pic)
    assert demo._render_palette(None, 20).shape == (20, 3)
    assert demo._render_palette(list(range(60)), 20).tolist() == np.arange(60).reshape(20, 3).tolist()
    with pytest.raises(ValueError, match="rows"):
        demo._render_palette(list(range(30)), 20)
