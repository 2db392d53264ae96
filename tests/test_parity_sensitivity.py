"""The parity criterion itself (tests/parity.py) on the CPU: built from the oracle alone, a candidate that is the fp32
oracle must pass it, and candidates wrong by a per cent in one frame, one layer, one tile or one object must not.  For
the first two errors the criterion before per-element noise (one tensor-wide noise maximum, a fraction of the
elements let through) is shown accepting them: the reason it was replaced."""
import pytest
import torch

from oracle import wif_oracle as O
from parity import TOL, close, compare_warp_composite

# cases of test_gpu_parity.py: the two fixed ones whose control-point bound was loosest (bound / scale 0.22 and
# 1.2e-4 with the noise maximum), the L = 17 one, and draw 15 of the seeded fuzz (x4-upsampled layers)
NL3 = dict(f=1, nl=3, h=96, w=256, sigma=0.3)
NL17 = dict(f=1, nl=17, h=16, w=32)
FUZZ15 = dict(f=3, nl=8, h=10, w=92, k=3, sigma=0.5, smooth=4, seed=1015, wseed=15)


def _case(cfg):
    """Oracle only: the fp32 oracle (the candidate, and m32: the fp32 oracle at its own coordinates), the plain fp64
    oracle (the `exact` of the criterion before), and m64: the fp64 oracle at the fp32 oracle's own pixel coordinates
    -- on the host they are the un-normalisation of its grid, the same expression in fp32."""
    f, nl, h, w, k = cfg["f"], cfg["nl"], cfg["h"], cfg["w"], cfg.get("k", 4)
    ctrl = O.get_grid(k, k).view(-1, 2)
    layers, pts, occ, inv, rep = O.make_synthetic(f, nl, h, w, k_side=k, seed=cfg.get("seed", nl),
                                                  sigma=cfg.get("sigma", 0.1), smooth=cfg.get("smooth", 0))
    torch.manual_seed(cfg.get("wseed", f * 100 + nl))
    w1, w2 = torch.randn(f, 3, h, w), torch.randn(f, nl, h, w)
    grid32 = O.tps_grid(inv, rep, pts, h, w)
    pos32 = torch.stack([((grid32[..., 0] + 1) * w - 1) / 2, ((grid32[..., 1] + 1) * h - 1) / 2], dim=-1)

    def run(dtype, pos=None):
        l, p, o = (x.detach().to(dtype).requires_grad_() for x in (layers, pts, occ))
        if pos is None:
            rgb, alpha = O.warp_composite(l, p, o, inv.to(dtype), rep.to(dtype), explicit=True)
        else:
            rgb, alpha = O.warp_composite_px(l, p, o, inv.to(dtype), rep.to(dtype), pos)
        ((rgb * w1.to(dtype)).sum() + (alpha * w2.to(dtype)).sum()).backward()
        return [rgb.detach(), alpha.detach(), l.grad, p.grad, o.grad]

    ref32 = run(torch.float32)
    # the hook at fp32 reproduces the fp32 oracle bit for bit: same coordinates, same arithmetic
    assert all(torch.equal(x, y) for x, y in zip(run(torch.float32, pos32), ref32))
    return ref32, run(torch.float64), run(torch.float64, pos32)


@pytest.fixture(scope="module")
def cases():
    return {name: _case(cfg) for name, cfg in (("nl3", NL3), ("nl17", NL17), ("fuzz15", FUZZ15))}


def _rejects(got, m32, m64):
    with pytest.raises(AssertionError):
        compare_warp_composite(got, m32, m64)


def _close_before(a, b, exact, rel, kink_fraction):
    """The criterion this suite used before: bound = TOL * max|b| + k * max|b - exact|, one number for the tensor,
    and a fraction of the elements allowed up to 25 x over it.  True when it accepts ``a``."""
    a, b, e = a.double(), b.double(), exact.double()
    scale = b.abs().max().item() if rel else 1.0
    bound = TOL * scale + (4.0 if rel else 2.0) * (b - e).abs().max().item()
    dev = torch.maximum((a - b).abs(), (a - e).abs())
    return (dev > bound).double().mean().item() <= kink_fraction and dev.max().item() <= 25 * bound


@pytest.mark.parametrize("name", ["nl3", "nl17", "fuzz15"])
def test_fp32_oracle_passes(cases, name):
    ref32, ref64, matched = cases[name]
    # (the candidate IS m32 here, so each first close() -- against m32 with its noise from m64 -- passes by
    # construction: err = 0 and |got - m64| is the noise itself.  What this checks is the second one, rgb, alpha and
    # grad_pts against m64 at plain TOL * scale; grad_layers and grad_occ are only checked by the rejections below.)
    compare_warp_composite(ref32, ref32, matched)
    # the bound on the control-point gradient is the plain north star, on every case
    scale = ref32[3].abs().max()
    assert (ref32[3].double() - matched[3]).abs().max() <= TOL * scale


def test_rejects_one_frame_of_grad_pts_off_by_one_percent(cases):
    ref32, ref64, matched = cases["nl3"]
    got = [x.clone() for x in ref32]
    nl = NL3["nl"]
    got[3][:nl] += 0.01 * ref32[3].abs().max()
    _rejects(got, ref32, matched)
    assert _close_before(got[3], ref32[3], ref64[3], rel=True, kink_fraction=0.05)


def test_rejects_the_smallest_layer_of_grad_layers_scaled_by_1_01(cases):
    ref32, ref64, matched = cases["nl17"]
    got = [x.clone() for x in ref32]
    per_layer = ref32[2].abs().amax(dim=(2, 3, 4))  # (F, L)
    f, l = divmod(int(per_layer.argmin()), per_layer.shape[1])
    assert per_layer[f, l] < 1e-2 * per_layer.max()  # a layer the tensor-wide scale does not see
    got[2][f, l] *= 1.01
    _rejects(got, ref32, matched)
    assert _close_before(got[2], ref32[2], ref64[2], rel=True, kink_fraction=0.05)


def test_rejects_a_zeroed_edge_tile_of_grad_layers(cases):
    ref32, ref64, matched = cases["nl3"]
    got = [x.clone() for x in ref32]
    tile = (slice(None), slice(None), slice(None), slice(-16, None), slice(-16, None))  # the last 16 x 16 tile
    per_layer = ref32[2][tile].abs().amax(dim=(2, 3, 4))
    f, l = divmod(int(per_layer.argmax()), per_layer.shape[1])
    assert per_layer[f, l] > 1e-3 * ref32[2].abs().max()  # it carries gradient
    got[2][f, l, :, -16:, -16:] = 0
    _rejects(got, ref32, matched)


@pytest.mark.parametrize("where", ["candidate", "reference"])
def test_rejects_a_single_nan(cases, where):
    """One NaN element -- a tail tile never written, uninitialised LDS, a 0/0 -- fails every output's comparison,
    wherever it sits, and close() rejects it in every mode."""
    ref32, _, matched = cases["nl3"]
    for i in range(5):
        got, m32 = [x.clone() for x in ref32], [x.clone() for x in ref32]
        (got if where == "candidate" else m32)[i].view(-1)[7] = float("nan")
        _rejects(got, m32, matched)
    one_nan = torch.ones(4)
    one_nan[1] = float("nan")
    a, b = (one_nan, torch.ones(4)) if where == "candidate" else (torch.ones(4), one_nan)
    for kw in ({}, dict(rel=True), dict(rel=True, exact=torch.ones(4)), dict(rel=True, slice_dims=(0,)),
               dict(exact=torch.ones(4), noise_of="tensor"), dict(exempt=torch.ones(4, dtype=torch.bool))):
        with pytest.raises(AssertionError):
            close(a, b, what="one NaN", **kw)


def test_rejects_one_object_class_gradient_off_by_half_a_percent():
    """The HD backward's class gradient, from the oracle alone (the num_obj = 10 layout-filter recipe of
    test_fused_hd_backward): the fp32 oracle passes close() with the per-object scale and kink mask of the GPU test,
    one object's row scaled by 1.005 does not."""
    from test_gpu_warper import HD_GRAD_NAMES, _HD_SLICES, _hd_kinks, _hd_oracle, opt_ns
    opt = opt_ns(include_self=False, num_obj=10, dim=16, load_dim=32, use_lyt_filtering=True, weight_cls=True,
                 min_cls=0.05)
    o = _hd_oracle(opt, True, False, b=2, t=3, nl=6, seed=17)
    i = HD_GRAD_NAMES.index("cls")
    g32, g64 = o.g_o[i], o.g_64[i]
    exempt = _hd_kinks(o.cfg, o.grid_o, o.inp, o.obj_alpha, o.bg_alpha, o.cls, o.ctx_ts, True).get("cls")
    close(g32, g32, rel=True, what="cls", exact=g64, slice_dims=_HD_SLICES["cls"], exempt=exempt)
    got = g32.clone()
    ok = ~exempt[..., 0] if exempt is not None else torch.ones(got.shape[:2], dtype=torch.bool)
    b, obj = [int(v) for v in ok.nonzero()[-1]]  # an object no kink exempts
    got[b, obj] *= 1.005
    with pytest.raises(AssertionError):
        close(got, g32, rel=True, what="cls", exact=g64, slice_dims=_HD_SLICES["cls"], exempt=exempt)
