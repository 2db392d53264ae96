"""GPU: deterministic mode (waldo_amd.set_deterministic, include/waldo_hip.h "Reproducible gradients").

Every gradient of the library is the same bits from run to run in that mode -- eagerly and replayed from a HIP graph --
and stays within the bounds the existing backward tests of the same ops hold the default mode to (their oracles,
their ``close`` arguments; the helpers are imported from those test modules so that nothing is restated).  Inputs are
smooth and seeded: no ``exempt=`` mask is used anywhere in this file."""

import pytest
import torch

from oracle import wif_oracle as O

pytestmark = pytest.mark.gpu

from parity import close  # noqa: E402

RUNS = 5


@pytest.fixture
def calls(monkeypatch):
    """Names of the entry points and size queries the library is asked for, in order."""
    from waldo_amd import _lib
    seen = []
    call, query = _lib.call, _lib.query

    def rec_call(name, *args):
        seen.append(name)
        return call(name, *args)

    def rec_query(name, *args):
        seen.append(name)
        return query(name, *args)

    monkeypatch.setattr(_lib, "call", rec_call)
    monkeypatch.setattr(_lib, "query", rec_query)
    return seen


@pytest.fixture
def torch_flag():
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def det_names(seen):
    return [n for n in seen if "_det" in n]


def same_bits(fn, what):
    """``fn() -> list of tensors``: RUNS evaluations in deterministic mode give the same bits; the default mode's are
    printed (information: asserting non-determinism would be flaky)."""
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        first = [g.clone() for g in fn()]
        for r in range(1, RUNS):
            for i, (a, b) in enumerate(zip(fn(), first)):
                assert torch.equal(a, b), f"{what}: gradient {i} of run {r} differs from run 0"
    with WF.deterministic(False):
        runs = [[g.clone() for g in fn()] for _ in range(RUNS)]
    differ = [i for i in range(len(first)) if any(not torch.equal(r[i], runs[0][i]) for r in runs[1:])]
    print(f"[deterministic] {what}: default mode, {RUNS} runs: "
          + (f"gradients {differ} differed" if differ else "no gradient differed"))
    for a in first:
        assert torch.isfinite(a).all() and a.abs().sum() > 0, what
    return first


# ------------------------------------------------------------------------------------------------ inputs
def _folded_grid(n, h, w, g, dev, spread=0.12):
    """Sample positions that fold the whole raster onto a few texels around the centre (a smooth map, plus a seeded
    per-map offset): thousands of outputs per texel."""
    ys = torch.linspace(-1, 1, h, device=dev).view(1, h, 1)
    xs = torch.linspace(-1, 1, w, device=dev).view(1, 1, w)
    off = (torch.rand(n, 1, 1, 2, generator=g, device=dev) - 0.5) * 0.3
    return torch.stack([(spread * torch.sin(3 * xs + ys)).expand(n, h, w),
                        (spread * torch.cos(2 * ys - xs)).expand(n, h, w)], dim=-1) + off


def _gs_case(dev, folded=True):
    """grid_sample with the time broadcast (lvd.py:544): b * no canvases of 8 x 8, each read by t output maps of
    32 x 64 pixels (8 workgroups per map)."""
    b, t, no, c, ho, wo, h, w = 2, 3, 4, 2, 8, 8, 32, 64
    g = torch.Generator(device=dev).manual_seed(11)
    obj = torch.randn(b * no, c, ho, wo, generator=g, device=dev)
    grid = _folded_grid(b * t * no, h, w, g, dev) if folded else \
        torch.rand(b * t * no, h, w, 2, generator=g, device=dev) * 2.2 - 1.1
    wgt = torch.randn(b * t * no, c, h, w, generator=g, device=dev)
    return obj, grid, wgt, (t * no, no)


def _gs_grads(obj, grid, wgt, bc, scale=1.0, wgt_edit=None):
    from waldo_amd import functional as WF
    o, gr = obj.clone().requires_grad_(), grid.clone().requires_grad_()
    out = WF.grid_sample(o, gr, delta=1.0, broadcast=bc)
    wg = wgt if wgt_edit is None else wgt_edit(wgt.clone())
    out.backward(wg * scale)
    return [o.grad, gr.grad]


def _fcw_case(dev, folded=True, ghost=True):
    """flow_ctx_warp at x2: 2 clips, 2 context x 2 predicted frames, 6 layers, 32 x 64 HD pixels (8 tiles: two
    workgroups per unit).  ``folded``: flows that send every pixel near the frame's centre."""
    b, t, tc, tp, nl, s, tw, h, w = 2, 3, 2, 2, 6, 2, 2, 16, 32
    hd, wd = h * s, w * s
    g = torch.Generator(device=dev).manual_seed(29)
    m = b * tc * tp
    flow_lr = 0.05 * torch.randn(m, nl, 2, h, w, generator=g, device=dev)
    if folded:
        ys = torch.linspace(-1, 1, h, device=dev).view(1, 1, h, 1).expand(m, nl, h, w)
        xs = torch.linspace(-1, 1, w, device=dev).view(1, 1, 1, w).expand(m, nl, h, w)
        flow_lr = flow_lr + torch.stack([-0.9 * xs, -0.9 * ys], dim=2)
    isobj = (torch.rand(m, nl - 1, h, w, generator=g, device=dev) > 0.3).float() if ghost else None
    lo = torch.rand(b * tw, nl, hd // 4, wd // 4, generator=g, device=dev)
    a01 = torch.nn.functional.interpolate(lo, size=(hd, wd), mode="bilinear")
    occ = torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5
    ctx_ts = torch.tensor([[[0, 1], [1, 1]], [[1, 0], [0, 0]]], device=dev)
    pred_ts = torch.tensor([2, 0], device=dev)
    ws = [torch.randn(m, 2, hd, wd, generator=g, device=dev), torch.randn(m, nl, hd, wd, generator=g, device=dev),
          torch.randn(m, hd, wd, generator=g, device=dev)]
    return (flow_lr, isobj, a01, ctx_ts, pred_ts, occ, tw, s), ws


def _fcw_grads(case, ws, scale=1.0, ws_edit=None):
    from waldo_amd import functional as WF
    flow_lr, isobj, a01, ctx_ts, pred_ts, occ, tw, s = case
    leaves = [x.clone().requires_grad_() for x in (flow_lr, a01, occ)]
    flow, actx, dis = WF.flow_ctx_warp(leaves[0], isobj, leaves[1], ctx_ts, pred_ts, leaves[2], tw, s)[:3]
    ws = ws if ws_edit is None else ws_edit([x.clone() for x in ws])
    torch.autograd.backward([flow, actx, dis], [x * scale for x in ws])
    return [x.grad for x in leaves]


def _fca_grads(dev):
    from waldo_amd import functional as WF
    b, t, tw, h, w, nl, s, ncls = 2, 3, 2, 16, 32, 9, 2, 20
    hd, wd = h * s, w * s
    g = torch.Generator(device=dev).manual_seed(44)
    alpha_lr = torch.rand(b * tw, nl, h, w, generator=g, device=dev)
    inp = torch.randn(b, t, 3 + ncls, hd, wd, generator=g, device=dev) * 2
    dist = torch.rand(b, nl - 1, ncls, generator=g, device=dev).softmax(dim=2)
    occ = torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5
    w1 = torch.randn(b * tw, nl, hd, wd, generator=g, device=dev)
    w2 = torch.randn(b * tw, nl, hd, wd, generator=g, device=dev)

    def run():
        leaves = [x.clone().requires_grad_() for x in (alpha_lr, dist, occ)]
        a01, alpha = WF.flow_ctx_alpha(leaves[0], inp, leaves[1], leaves[2], tw, 3, s)
        ((a01 * w1).sum() + (alpha * w2).sum()).backward()
        return [x.grad for x in leaves]
    return run


def _wc_case(dev, f=2, nl=8, h=64, w=96, seed=21, dtype=torch.float32):
    import waldo_amd
    layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=seed, smooth=8)
    tps = waldo_amd.TPSWarp(h, w, O.get_grid(4, 4).view(-1, 2)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    w1 = torch.randn(f, 3, h, w, generator=g, device=dev)
    w2 = torch.randn(f, nl, h, w, generator=g, device=dev)
    return layers.to(dev, dtype), pts.to(dev), occ.to(dev), tps, w1, w2


def _wc_grads(case):
    from waldo_amd import functional as WF
    layers, pts, occ, tps, w1, w2 = case
    leaves = [x.clone().requires_grad_() for x in (layers, pts, occ)]
    rgb, alpha = WF.warp_composite(*leaves, tps.inverse_kernel, tps.basis_t, return_alpha=True)
    ((rgb * w1).sum() + (alpha * w2).sum()).backward()
    return [x.grad for x in leaves]


# ------------------------------------------------------------------------------------------------ 1. same bits
def test_same_bits_grid_sample_collisions_and_time_broadcast(dev, calls):
    obj, grid, wgt, bc = _gs_case(dev)
    same_bits(lambda: _gs_grads(obj, grid, wgt, bc), "grid_sample, folded grid, broadcast over time")
    assert "waldo_grid_sample2d_bwd_det" in calls and "waldo_grid_sample2d_bwd" in calls


def test_same_bits_layers_to_output(dev, calls):
    from waldo_amd import functional as WF
    b, t, no, c, ho, wo, h, w = 2, 3, 4, 2, 8, 8, 32, 64
    g = torch.Generator(device=dev).manual_seed(5)
    obj = torch.randn(b * no, c, ho, wo, generator=g, device=dev)
    bg = torch.randn(b, c, h, w, generator=g, device=dev)
    gobj, gbg = _folded_grid(b * t * no, h, w, g, dev), _folded_grid(b * t, h, w, g, dev, spread=0.5)
    wgt = torch.randn(b * t, no + 1, c, h, w, generator=g, device=dev)

    def run():
        leaves = [x.clone().requires_grad_() for x in (obj, bg, gobj, gbg)]
        out = WF.layers_to_output(*leaves, 1.0, 1.0, (t * no, no), (t, 1), (0.5, 0.5))
        (out * wgt).sum().backward()
        return [x.grad for x in leaves]

    same_bits(run, "layers_to_output")
    assert "waldo_grid_sample2d_ex_bwd_det" in calls


def test_same_bits_small_tables(dev, calls):
    from waldo_amd import functional as WF
    import waldo_amd
    g = torch.Generator(device=dev).manual_seed(8)
    # occ_composite: 6 maps of 64 x 64 (16 tiles: four workgroups per map), three maps per matrix
    alpha = torch.rand(6, 9, 64, 64, generator=g, device=dev)
    occ = torch.rand(2, 9, 9, generator=g, device=dev)
    wgt = torch.randn(6, 9, 64, 64, generator=g, device=dev)

    def occ_run():
        a, o = alpha.clone().requires_grad_(), occ.clone().requires_grad_()
        (WF.occ_composite(a, o, occ_div=3) * wgt).sum().backward()
        return [a.grad, o.grad]

    same_bits(occ_run, "occ_composite")
    # tps_grid: K3 = 19 and the background's 131, 64 x 128 pixels (8 chunks: two workgroups per map)
    for ctrl in (O.get_grid(4, 4).view(-1, 2), O.get_grid(8, 16).view(-1, 2)):
        mod = waldo_amd.TPSWarp(64, 128, ctrl).to(dev)
        pts = ctrl.to(dev).view(1, -1, 2) + 0.02 * torch.randn(10, ctrl.shape[0], 2, generator=g, device=dev)
        wg = torch.randn(10, 64, 128, 2, generator=g, device=dev)

        def tps_run():
            p = pts.clone().requires_grad_()
            (mod(p) * wg).sum().backward()
            return [p.grad]

        same_bits(tps_run, f"tps_grid, {ctrl.shape[0]} control points")
    same_bits(_fca_grads(dev), "flow_ctx_alpha")
    for name in ("waldo_occ_composite_bwd_det", "waldo_tps_grid_bwd_det", "waldo_flow_ctx_alpha_bwd_det",
                 "waldo_tps_mapping_bwd"):
        assert name in calls, name


def test_same_bits_flow_ctx_warp_collisions(dev, calls):
    case, ws = _fcw_case(dev)
    same_bits(lambda: _fcw_grads(case, ws), "flow_ctx_warp, folded flows")
    assert "waldo_flow_ctx_warp_bwd_det" in calls


def test_same_bits_warp_composite_and_wif_fuse(dev, calls):
    from waldo_amd import functional as WF
    case = _wc_case(dev)
    same_bits(lambda: _wc_grads(case), "warp_composite with grad_occ")
    assert "waldo_warp_composite_bwd_det" in calls
    g = torch.Generator(device=dev).manual_seed(2)
    vid = torch.randn(1, 2, 2, 5, 32, 64, generator=g, device=dev)
    net = torch.randn(1, 2, 2, 5, 32, 64, generator=g, device=dev)
    wgt = torch.randn(1, 2, 3, 32, 64, generator=g, device=dev)

    def wif_run():
        v, n = vid.clone().requires_grad_(), net.clone().requires_grad_()
        (WF.wif_fuse(v, n) * wgt).sum().backward()
        return [v.grad, n.grad]

    same_bits(wif_run, "wif_fuse (no atomics)")


def _lvd_grads(step):
    loss = step()
    return [loss.detach().clone()] + [x.grad.clone() for x in step.leaves]


def test_same_bits_lvd_step_covers_the_ops_that_need_nothing(dev, calls):
    """The LVD step's backward runs inverse_warp, time_gather, lyt_dist, frame_warp_fuse, compute_occ, alpha_head,
    pose_affine and tps_mapping (no atomics: nothing to replace) next to the replaced ones: all of it, five times."""
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(1, dev, seed=3)
    same_bits(lambda: _lvd_grads(step), "LvdStep(clips=1)")
    for name in ("waldo_inverse_warp_bwd", "waldo_lyt_dist_bwd", "waldo_frame_warp_fuse_bwd", "waldo_compute_occ_bwd",
                 "waldo_alpha_head_bwd", "waldo_pose_affine_bwd", "waldo_tps_mapping_bwd", "waldo_tps_grid_bwd_det",
                 "waldo_grid_sample2d_ex_bwd_det", "waldo_flow_ctx_alpha_bwd_det", "waldo_flow_ctx_warp_bwd_det"):
        assert name in calls, name


# ------------------------------------------------------------------------------------------------ 2. right values
def test_right_values_grid_sample(dev, calls):
    """tests/test_gpu_parity.py::test_grid_sample_random / _broadcast, in deterministic mode."""
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        for n, c, hi, wi, ho, wo in ((4, 2, 64, 64, 128, 256), (2, 2, 128, 256, 40, 32), (2, 3, 7, 5, 300, 1)):
            torch.manual_seed(n * 7 + c)
            x = torch.randn(n, c, hi, wi, requires_grad=True)
            grid = (torch.rand(n, ho, wo, 2) * 2.4 - 1.2).requires_grad_()
            ref = O.grid_sample_delta(x, grid, 0.5)
            wgt = torch.randn(ref.shape)
            (ref * wgt).sum().backward()
            x2, g2 = x.detach().to(dev).requires_grad_(), grid.detach().to(dev).requires_grad_()
            out = WF.grid_sample(x2, g2, delta=0.5)
            close(out, ref, what="out")
            (out * wgt.to(dev)).sum().backward()
            close(x2.grad, x.grad, rel=True, what="grad_x")
            close(g2.grad, grid.grad, rel=True, what="grad_grid")
        b, t, no, c, ho, wo, h, w = 2, 3, 4, 2, 8, 8, 12, 10
        torch.manual_seed(3)
        obj = torch.randn(b, no, c, ho, wo, requires_grad=True)
        grid = (torch.rand(b * t * no, h, w, 2) * 2.2 - 1.1)
        exp = obj.view(b, 1, no, c, ho, wo).expand(-1, t, -1, -1, -1, -1).reshape(b * t * no, c, ho, wo)
        ref = O.grid_sample_delta(exp, grid, 1.0)
        wgt = torch.randn(ref.shape)
        (ref * wgt).sum().backward()
        o2 = obj.detach().to(dev).requires_grad_()
        out = WF.grid_sample(o2.view(b * no, c, ho, wo), grid.to(dev), delta=1.0, broadcast=(t * no, no))
        (out * wgt.to(dev)).sum().backward()
        close(o2.grad, obj.grad, rel=True, what="grad_obj")
        # the folded grid of the reproducibility test: thousands of contributions per texel
        objd, gridd, wgtd, bc = _gs_case(dev)
        got = _gs_grads(objd, gridd, wgtd, bc)
        oc = objd.cpu().requires_grad_()
        exp = oc.view(b, 1, no, c, ho, wo).expand(-1, t, -1, -1, -1, -1).reshape(b * t * no, c, ho, wo)
        (O.grid_sample_delta(exp, gridd.cpu(), 1.0) * wgtd.cpu()).sum().backward()
        close(got[0], oc.grad, rel=True, what="grad_obj, folded grid")
    assert calls.count("waldo_grid_sample2d_bwd_det") == 5 and "waldo_grid_sample2d_bwd" not in calls


@pytest.mark.parametrize("hwo,shared", [((16, 32), True), ((12, 10), False)])
def test_right_values_layers_to_output(dev, calls, hwo, shared):
    import test_gpu_parity as tp
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tp.test_layers_to_output_is_the_concatenation(dev, hwo, shared)
    assert "waldo_grid_sample2d_ex_bwd_det" in calls and "waldo_grid_sample2d_ex_bwd" not in calls


@pytest.mark.parametrize("nl", [5, 9, 17, 32])
def test_right_values_occ_composite(dev, calls, nl):
    import test_gpu_parity as tp
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tp.test_occ_composite(dev, nl)
    assert "waldo_occ_composite_bwd_det" in calls and "waldo_occ_composite_bwd" not in calls


def test_right_values_tps(dev, calls):
    import test_gpu_parity as tp
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tp.test_tps_bg_sized(dev)
    assert "waldo_tps_grid_bwd_det" in calls and "waldo_tps_grid_bwd" not in calls


def test_right_values_flow_ctx_alpha(dev, calls):
    import test_gpu_warper as tw
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tw.test_flow_ctx_alpha_backward_takes_both_output_gradients(dev, 17, 1, 21)
        tw.test_flow_ctx_alpha_backward_takes_both_output_gradients(dev, 5, 2, 20)
    assert "waldo_flow_ctx_alpha_bwd_det" in calls and "waldo_flow_ctx_alpha_bwd" not in calls


@pytest.mark.parametrize("over,ctx_only,include_self", [
    (dict(num_obj=3, dim=16, load_dim=0), False, True),
    (dict(num_obj=16, obj_shape=[2, 2], dim=8, load_dim=32), True, False),
    (dict(num_obj=10, dim=16, load_dim=32, use_lyt_filtering=True, weight_cls=True, min_cls=0.05), True, False),
])
def test_right_values_fused_hd_backward(dev, calls, over, ctx_only, include_self):
    """tests/test_gpu_warper.py::test_fused_hd_backward's oracle comparison (fp32 and fp64, every differentiable
    input of grid_to_flow[_ctx] -> input_to_output), in deterministic mode."""
    import test_gpu_warper as tw
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tw._hd_backward_case(dev, tw.opt_ns(include_self=include_self, **over), ctx_only, include_self, b=2, t=3, nl=6,
                             seed=17, per_op=False)
    for name in ("waldo_flow_ctx_alpha_bwd_det", "waldo_flow_ctx_warp_bwd_det", "waldo_grid_sample2d_ex_bwd_det"):
        assert name in calls, name
    assert "waldo_flow_ctx_warp_bwd" not in calls


def test_right_values_fused_hd_backward_at_recipe_size(dev, calls):
    import test_gpu_warper as tw
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tw.test_fused_hd_backward_at_recipe_size(dev)
    assert "waldo_flow_ctx_warp_bwd_det" in calls and "waldo_flow_ctx_warp_bwd" not in calls


def test_right_values_warp_composite(dev, calls):
    """tests/test_gpu_parity.py::test_warp_composite_smooth_is_strict and the matched-coordinates comparison of
    test_c3_eight_frames_with_grad_occ on the same smooth input, in deterministic mode."""
    import test_gpu_parity as tp
    from waldo_amd import functional as WF
    with WF.deterministic(True):
        tp.test_warp_composite_smooth_is_strict(dev)
        f, nl, h, w = 2, 8, 128, 128
        layers, pts, occ, _, _ = O.make_synthetic(f, nl, h, w, seed=13, smooth=8)
        ctrl = O.get_grid(4, 4).view(-1, 2)
        hip = tp._hip_fused(dev, layers, pts, occ, ctrl, None, None, "sq")
        tp._compare_fused(hip, *tp._matched(dev, layers, pts, occ, ctrl, None, None, "sq"))
    assert calls.count("waldo_warp_composite_bwd_det") == 2 and "waldo_warp_composite_bwd" not in calls


# ------------------------------------------------------------------------------------------------ 3. exactly linear
def test_splats_are_exactly_linear(dev):
    from waldo_amd import functional as WF
    obj, grid, wgt, bc = _gs_case(dev)
    case, ws = _fcw_case(dev)
    with WF.deterministic(True):
        for what, fn, idx in (("grid_sample grad_input", lambda s: _gs_grads(obj, grid, wgt, bc, s), 0),
                              ("flow_ctx_warp grad_a01", lambda s: _fcw_grads(case, ws, s), 1)):
            g1, g2, g3 = fn(1.0)[idx], fn(2.0)[idx], fn(3.0)[idx]
            assert g1.abs().sum() > 0
            assert torch.equal(g2, 2 * g1), f"{what}: loss x 2 is not gradient x 2 bit for bit"
            close(g3, 3 * g1, rel=True, what=f"{what}: loss x 3")


# ------------------------------------------------------------------------------------------------ 4. training steps
def test_lvd_step_under_torch_deterministic_algorithms(dev, calls, torch_flag):
    """LvdStep(clips=2) with torch.use_deterministic_algorithms(True) and the library's mode left at None: no framework
    op on the fused path is without a deterministic implementation, and two steps from fresh leaves agree bit for bit."""
    from waldo_amd import functional as WF
    from waldo_amd.tools.lvd_step import LvdStep
    WF.set_deterministic(None)
    torch.use_deterministic_algorithms(True)
    a = _lvd_grads(LvdStep(2, dev, seed=1))
    b = _lvd_grads(LvdStep(2, dev, seed=1))
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"loss / leaf gradient {i} differs between two steps from the same seed"
        assert torch.isfinite(x).all()
    assert det_names(calls) and "waldo_flow_ctx_warp_bwd" not in calls and "waldo_grid_sample2d_ex_bwd" not in calls


def _hd_step(dev, scale=4):
    """A full-resolution backward through decode_output at a small HD size (x4: the fused HD backward kernels)."""
    import test_gpu_warper as tw
    from oracle import warper_oracle as WO
    from waldo_amd.nets import Warper, decode_output
    opt = tw.opt_ns(num_obj=5, dim=16, load_dim=16 * scale, use_lyt_filtering=True, weight_cls=True, min_cls=0.05)
    cfg = WO.WarperCfg.from_opt(opt)
    wp = Warper(opt).to(dev)
    b, t, nl = 2, 3, 6
    obj_pose, bg_pose, inp, occ, obj_alpha, bg_alpha, cls = tw._warper_inputs(cfg, b, t, nl, seed=31)
    ctx_ts = torch.tensor([[[0], [1]], [[1], [1]]], device=dev)
    pred_ts = torch.tensor([2], device=dev)

    def run():
        leaves = [x.clone().to(dev).requires_grad_() for x in (obj_pose, bg_pose, occ, obj_alpha, cls)]
        op, bp, oc, oa, cl = leaves
        grid = wp(op, bp)
        out = decode_output(wp, inp.to(dev), grid, oc, oa, bg_alpha.to(dev), cl, ctx_ts, pred_ts)
        loss = sum(x.square().mean() for x in out if torch.is_tensor(x) and x.requires_grad)
        loss.backward()
        return [loss.detach()] + [x.grad for x in leaves]
    return run


def test_hd_decode_and_c3_under_torch_deterministic_algorithms(dev, calls, torch_flag):
    from waldo_amd import functional as WF
    WF.set_deterministic(None)
    torch.use_deterministic_algorithms(True)
    run = _hd_step(dev)
    for i, (x, y) in enumerate(zip(run(), run())):
        assert torch.equal(x, y), f"decode_output x4: loss / gradient {i}"
    assert "waldo_flow_ctx_warp_bwd_det" in calls and "waldo_flow_ctx_alpha_bwd_det" in calls
    # BASELINE C3's shape with the composited alpha and a gradient on occ, fp32 and bf16 layers
    for dtype in (torch.float32, torch.bfloat16):
        case = _wc_case(dev, f=16, nl=8, h=256, w=512, seed=5, dtype=dtype)
        a, b = _wc_grads(case), _wc_grads(case)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"C3 {dtype}: gradient {i}"
            assert torch.isfinite(x.float()).all() and x.float().abs().sum() > 0
        assert a[0].dtype == dtype
    assert calls.count("waldo_warp_composite_bwd_det") == 4


# ------------------------------------------------------------------------------------------------ 5. from a graph
def test_lvd_step_replayed_from_a_graph(dev, torch_flag):
    """Captured as bench.py --config LVD --graph captures it: each replay equals the eager deterministic step bit for
    bit -- every leaf gradient (the graph's buffers, poisoned before each replay so that a replay must write all of
    them) and the loss -- so the mode neither synchronises nor reads anything back.

    The loss is compared through a copy taken INSIDE the captured graph.  In a capture that ends with ``step()`` itself
    (bench.py's form) the 0-dim tensor it returns read back -0.4442 after the first replay (the eager value) and 0.1199
    -- NaN under torch.use_deterministic_algorithms -- after every later one, while every gradient of the same replays
    had the eager bits: measured with the mode off as well, i.e. on the kernels of the parent commit, so it is not a
    property of this mode.  With the copy in the capture both tensors read the eager value (printed below)."""
    from waldo_amd import _lib, functional as WF
    from waldo_amd.tools.lvd_step import LvdStep
    WF.set_deterministic(None)
    torch.use_deterministic_algorithms(True)
    eager = _lvd_grads(LvdStep(2, dev, seed=1))
    step = LvdStep(2, dev, seed=1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        kept = loss.detach().clone()
    for r in range(3):
        for x in step.leaves:
            x.grad.fill_(float("nan"))  # (the graph's buffers: every replay must write all of them)
        kept.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        print(f"[deterministic] replay {r}: loss {float(kept):.9g}, the tensor step() returned reads {float(loss.detach()):.9g}, "
              f"eager {float(eager[0]):.9g}")
        got = [kept] + [x.grad for x in step.leaves]
        for i, (x, y) in enumerate(zip(got, eager)):
            assert torch.equal(x, y), f"replay {r}: loss / leaf gradient {i} differs from the eager step"
    _lib.IndexStatus.check_all(sync=True)


# ------------------------------------------------------------------------------------------------ 6. bound at forward
def test_mode_is_bound_when_the_forward_runs(dev, calls):
    from waldo_amd import functional as WF
    obj, grid, wgt, bc = _gs_case(dev)
    case, ws = _fcw_case(dev)

    def forward():
        o = obj.clone().requires_grad_()
        out = WF.grid_sample(o, grid, delta=1.0, broadcast=bc)
        flow_lr, isobj, a01, ctx_ts, pred_ts, occ, tw, s = case
        a = a01.clone().requires_grad_()
        res = WF.flow_ctx_warp(flow_lr, isobj, a, ctx_ts, pred_ts, occ, tw, s)
        return (o, a), (out * wgt).sum() + (res[1] * ws[1]).sum()

    WF.set_deterministic(False)
    try:
        with WF.deterministic(True):
            leaves, loss = forward()
        del calls[:]
        loss.backward()  # outside the block
        assert sorted(det_names(calls)) == ["waldo_flow_ctx_warp_bwd_det", "waldo_flow_ctx_warp_bwd_det_workspace_bytes",
                                            "waldo_grid_sample2d_bwd_det", "waldo_grid_sample2d_bwd_det_workspace_bytes"]
        first = [x.grad.clone() for x in leaves]
        with WF.deterministic(True):
            leaves, loss = forward()
        loss.backward()
        assert all(torch.equal(x.grad, y) for x, y in zip(leaves, first))
        leaves, loss = forward()  # default mode
        del calls[:]
        with WF.deterministic(True):
            loss.backward()
        assert not det_names(calls) and "waldo_grid_sample2d_bwd" in calls and "waldo_flow_ctx_warp_bwd" in calls
    finally:
        WF.set_deterministic(None)


# ------------------------------------------------------------------------------------------------ 7. non-finite
def _planes_nan_or_equal(got, clean, nan_planes, what):
    """(P, ...) planes: those of ``nan_planes`` all NaN, every other one the bits of the clean run."""
    for p in range(got.shape[0]):
        if p in nan_planes:
            assert torch.isnan(got[p]).all(), f"{what}: plane {p} is reached by the NaN and must be all NaN"
        else:
            assert torch.equal(got[p], clean[p]), f"{what}: plane {p} is not reached by the NaN and must not change"


def test_non_finite_incoming_gradient_poisons_its_plane_only(dev):
    from waldo_amd import functional as WF
    obj, grid, wgt, bc = _gs_case(dev)
    case, ws = _fcw_case(dev, ghost=False)
    with WF.deterministic(True):
        clean = _gs_grads(obj, grid, wgt, bc)[0]
        n, ch = 17, 1  # output map 17 = (b 1, t 1, object 1) reads canvas b * no + object = 5

        def edit(wg):
            wg[n, ch, 7, 9] = float("nan")
            return wg
        got = _gs_grads(obj, grid, wgt, bc, wgt_edit=edit)[0]
        c = obj.shape[1]
        _planes_nan_or_equal(got.flatten(0, 1), clean.flatten(0, 1), {5 * c + ch}, "grid_sample grad_input")

        clean = _fcw_grads(case, ws)[1]
        m, layer = 5, 2  # unit 5 = (b 1, tc 0, tp 1) samples context frame ctx_ts[1, 0, 1] = 0: planes (1, 0, *)

        def edit_ws(w3):
            w3[1][m, layer, 11, 13] = float("nan")
            return w3
        got = _fcw_grads(case, ws, ws_edit=edit_ws)[1]
        nl, tw = got.shape[1], 2
        reach = {(1 * tw + 0) * nl + l for l in range(nl)}  # (the composite's backward spreads it over the layers)
        _planes_nan_or_equal(got.flatten(0, 1), clean.flatten(0, 1), reach, "flow_ctx_warp grad_a01")


# ------------------------------------------------------------------------------------------------ 8. no silent fallback
def test_unserved_shape_raises_from_the_forward(dev, calls):
    from waldo_amd import _lib, functional as WF
    case = _wc_case(dev, f=1, nl=24, h=32, w=32)
    layers, pts, occ, tps, w1, w2 = case
    with WF.deterministic(True):
        with pytest.raises(_lib.WaldoHipError, match="warp_composite: no deterministic kernel"):
            WF.warp_composite(layers.clone().requires_grad_(), pts, occ, tps.inverse_kernel, tps.basis_t)
        with torch.no_grad():  # no gradient required: the forward is served
            WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)
    assert not any(n.startswith("waldo_warp_composite_bwd") and "workspace" not in n for n in calls)
    with WF.deterministic(False):
        grads = _wc_grads(case)
    assert all(torch.isfinite(g).all() for g in grads) and "waldo_warp_composite_bwd" in calls


# ------------------------------------------------------------------------------------------------ 9. default untouched
def test_default_mode_calls_no_det_entry_point(dev, calls):
    import test_gpu_warper as tw
    from waldo_amd import functional as WF
    from waldo_amd.tools.lvd_step import LvdStep
    with WF.deterministic(False):
        step = LvdStep(1, dev, seed=0)
        step()
        assert step.grads_finite()
        # the LVD recipe's backward against the oracle, as tests/test_gpu_warper.py requires of the default mode
        tw.test_fused_hd_backward_at_recipe_size(dev)
    assert not det_names(calls), det_names(calls)
    for name in ("waldo_flow_ctx_warp_bwd", "waldo_flow_ctx_alpha_bwd", "waldo_grid_sample2d_ex_bwd", "waldo_tps_grid_bwd"):
        assert name in calls, name


# ------------------------------------------------------------------------------------------------ 10. one body, two modes
# The atomic and the deterministic entry point of an op share one host body: the branches of those bodies that no test
# above reaches, each on both paths, against the oracle in float64 (autograd on the CPU, from the same fp32 inputs).
def _oracle64(fn, inputs, wrt, weights):
    """Gradients of sum_k (fn(*inputs)[k] * weights[k]).sum() with respect to inputs[i], i in wrt, in float64."""
    xs = [x.double() if torch.is_tensor(x) and x.is_floating_point() else x for x in inputs]
    for i in wrt:
        xs[i].requires_grad_()
    outs = fn(*xs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * w.double()).sum() for o, w in zip(outs, weights)).backward()
    grads = [xs[i].grad for i in wrt]
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads), "the oracle's gradients must say something"
    return grads


def _both_paths(what, run, want, calls, names):
    """``run() -> gradients`` on the atomic and on the deterministic path, each against ``want``; the deterministic one
    gives the same bits twice."""
    from waldo_amd import functional as WF
    for det in (False, True):
        with WF.deterministic(det):
            got = run()
            for i, (g, w) in enumerate(zip(got, want)):
                close(g, w, rel=True, what=f"{what}, {'deterministic' if det else 'atomic'}: gradient {i}")
            if det:
                for i, (a, b) in enumerate(zip(run(), got)):
                    assert torch.equal(a, b), f"{what}: gradient {i} differs between two deterministic calls"
    for name in names:
        assert name in calls and name + "_det" in calls, name


def _flow_ctx_alpha_spelled_out(alpha_lr, inp, dist, occ, tw, s):
    """lvd.py:731-766 with framework ops (tests/test_gpu_warper.py::test_flow_ctx_alpha_skips_absent_layers_exactly's
    statement; ``dist`` None: no layout filter)."""
    import torch.nn.functional as F
    b = inp.shape[0]
    n, nl, h, w = alpha_lr.shape
    a = F.interpolate(alpha_lr, scale_factor=s, mode="bilinear") if s > 1 else alpha_lr
    if dist is not None:
        ncls = dist.shape[2]
        prob = inp[:, :tw, 3:].softmax(dim=2).reshape(n, 1, ncls, h * s, w * s)
        d = dist.view(b, 1, nl - 1, ncls, 1, 1).expand(-1, tw, -1, -1, -1, -1).reshape(n, nl - 1, ncls, 1, 1)
        a = torch.cat([a[:, :1], a[:, 1:] * (1 - (d - prob).abs().sum(dim=2) / 2)], dim=1)
    oc = occ[:, :tw].reshape(n, nl, nl)
    prod = torch.ones_like(a)
    for i in range(nl):
        prod = prod * (1 - a[:, i:i + 1] * oc[:, i].view(n, nl, 1, 1))
    return a * prod, a * prod * 2 - 1


def _short_window_clip(s, seed):
    """One clip of T = 3 frames of which the window holds Tw = 2; L = 3 layers; 4 x 6 pixels upsampled x s."""
    b, t, tw, nl, h, w, ncls = 1, 3, 2, 3, 4, 6, 5
    hd, wd = h * s, w * s
    g = torch.Generator().manual_seed(seed)
    alpha_lr = torch.rand(b * tw, nl, h, w, generator=g)
    inp = torch.randn(b, t, 3 + ncls, hd, wd, generator=g) * 2
    dist = torch.rand(b, nl - 1, ncls, generator=g).softmax(dim=2)
    occ = torch.rand(b, t, nl, nl, generator=g) * 0.5
    return (b, t, tw, nl, h, w, hd, wd), g, alpha_lr, inp, dist, occ


def test_one_body_grid_sample_gradient_of_the_grid_alone(dev, calls):
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(61)
    x = torch.randn(3, 2, 5, 7, generator=g)
    grid = torch.rand(3, 6, 5, 2, generator=g) * 2.4 - 1.2
    wgt = torch.randn(3, 2, 6, 5, generator=g)
    want = _oracle64(lambda a, b: O.grid_sample_delta(a, b, 0.5), (x, grid), (1,), (wgt,))

    def run():
        gr = grid.to(dev).requires_grad_()
        (WF.grid_sample(x.to(dev), gr, delta=0.5) * wgt.to(dev)).sum().backward()
        return [gr.grad]

    _both_paths("grid_sample, grad_grid alone", run, want, calls, ("waldo_grid_sample2d_bwd",))


def test_one_body_occ_composite_last_matrix_read_by_one_map(dev, calls):
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(62)
    alpha = torch.rand(3, 3, 300, generator=g)       # M = 3 maps of two tiles, the second partial
    occ = torch.rand(2, 3, 3, generator=g)           # occ_div = 2: matrix 1 is read by map 2 alone
    wgt = torch.randn(3, 3, 300, generator=g)
    want = _oracle64(lambda a, o: O.occlusion_product(a.unsqueeze(-1), o.repeat_interleave(2, dim=0)[:3]).squeeze(-1),
                     (alpha, occ), (0, 1), (wgt,))

    def run():
        a, o = alpha.to(dev).requires_grad_(), occ.to(dev).requires_grad_()
        (WF.occ_composite(a, o, occ_div=2) * wgt.to(dev)).sum().backward()
        return [a.grad, o.grad]

    _both_paths("occ_composite, occ_div 2 of 3 maps", run, want, calls, ("waldo_occ_composite_bwd",))


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("filtered", [False, True])
def test_one_body_flow_ctx_alpha_window_shorter_than_the_clip(dev, calls, s, filtered):
    from waldo_amd import functional as WF
    (b, t, tw, nl, h, w, hd, wd), g, alpha_lr, inp, dist, occ = _short_window_clip(s, 63)
    w1, w2 = torch.randn(b * tw, nl, hd, wd, generator=g), torch.randn(b * tw, nl, hd, wd, generator=g)
    if filtered:
        want = _oracle64(lambda a, d, o: _flow_ctx_alpha_spelled_out(a, inp.double(), d, o, tw, s), (alpha_lr, dist, occ),
                         (0, 1, 2), (w1, w2))
    else:
        want = _oracle64(lambda a, o: _flow_ctx_alpha_spelled_out(a, inp.double(), None, o, tw, s), (alpha_lr, occ), (0, 1),
                         (w1, w2))
    assert want[-1][:, tw:].abs().sum() == 0 and want[-1][:, :tw].abs().sum() > 0

    def run():
        leaves = [x.to(dev).requires_grad_() for x in ((alpha_lr, dist, occ) if filtered else (alpha_lr, occ))]
        a01, alpha = WF.flow_ctx_alpha(leaves[0], inp.to(dev), leaves[1] if filtered else None, leaves[-1], tw, 3, s)
        ((a01 * w1.to(dev)).sum() + (alpha * w2.to(dev)).sum()).backward()
        assert torch.equal(leaves[-1].grad[:, tw:], torch.zeros_like(leaves[-1].grad[:, tw:])), \
            "grad_occ: a frame outside the window receives nothing"
        return [x.grad for x in leaves]

    _both_paths(f"flow_ctx_alpha x{s}, Tw < T, {'layout filter' if filtered else 'no filter'}", run, want, calls,
                ("waldo_flow_ctx_alpha_bwd",))


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("leaf", ["a01", "occ"])
def test_one_body_flow_ctx_warp_one_gradient_required(dev, calls, s, leaf):
    import test_gpu_warper as tw_
    from waldo_amd import functional as WF
    (b, t, tw, nl, h, w, hd, wd), g, _, _, _, occ = _short_window_clip(s, 64)
    tc, tp = 2, 2
    m = b * tc * tp
    flow_lr = 0.3 * torch.randn(m, nl, 2, h, w, generator=g)
    isobj = (torch.rand(m, nl - 1, h, w, generator=g) > 0.3).float()
    a01 = torch.rand(b * tw, nl, hd, wd, generator=g)
    ctx_ts, pred_ts = torch.tensor([[[0, 1], [1, 0]]]), torch.tensor([2, 0])
    ws = (torch.randn(m, 2, hd, wd, generator=g), torch.randn(m, nl, hd, wd, generator=g),
          torch.randn(m, hd, wd, generator=g))
    args = (flow_lr, isobj, a01, ctx_ts, pred_ts, occ, tw, s)
    at = 2 if leaf == "a01" else 5
    want = _oracle64(tw_._flow_ctx_warp_spelled_out, args, (at,), ws)

    def run():
        xs = [x.to(dev) if torch.is_tensor(x) else x for x in args]
        xs[at] = xs[at].requires_grad_()
        outs = WF.flow_ctx_warp(*xs)[:3]
        sum((o * wk.to(dev)).sum() for o, wk in zip(outs, ws)).backward()
        return [xs[at].grad]

    _both_paths(f"flow_ctx_warp x{s}, only {leaf} requires a gradient", run, want, calls, ("waldo_flow_ctx_warp_bwd",))
